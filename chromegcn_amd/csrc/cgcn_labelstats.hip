// chromegcn_amd/csrc/cgcn_labelstats.hip
//
// Label and Hi-C neighbourhood statistics (scripts/analyze_results.py:226-266 get_label_weights, utils/util_methods.py:24-74
// summarize_data): exact integer counts over tensors that already live on the device (chromegcn_amd/labelstats.py, DESIGN.md
// section 4.13).  With P_c the windows u with targets[u, c] != 0 (the ablation's rule; NaN is positive):
//   window statistics   label_count[c] = |P_c|,  labels_hist[k] = windows with exactly k labels,  cooccurrence[a, b] = |P_a & P_b|
//   graph statistics    a neighbour entry is a stored (u, v) with u != v and (where the graph has values) val > 0;
//                       deg[u] = neighbour entries of row u,  n_entries = sum deg,  degree_sum[c] = sum over P_c of deg,
//                       contact_pairs[a, b] = neighbour entries (u, v) with u in P_a and v in P_b
// Passes:
//   k_ls_pack   one wavefront reads 64 consecutive labels of a row and ballots them into one 64-bit word: bits[n][W],
//               W = (C + 63) / 64 (bits past C are 0)
//   k_ls_pass   <GRAPH = false> window pass, <GRAPH = true> graph pass: ONE body.  Per row the wave forms nb[b], lane l owning
//               the labels l, l + 64, ...: the row's own bits (window pass; deg = 1) or the number of the row's neighbour entries
//               whose window carries b (graph pass: the 64 entries of a batch are read side by side, their words handed round
//               with readlane).  It then adds nb into row a of an LDS slab for every label a the row carries, and deg to an LDS
//               degree counter of a.  A C x C slab of 32-bit counters does not fit at C = 256, so the a-range is tiled over
//               grid.y: LS_AT = 32 labels x (64 W) x 4 B <= 32 KB, which leaves room for several workgroups per CU.  Rows of at
//               most LS_LONG entries go to one wave each; a longer row (hub rows of top-K graphs hold thousands) is split
//               over the workgroup's waves in 64-entry batches, every wave adding its own partial nb -- addition is linear,
//               so the waves never wait for each other.  Tile 0 also counts n_entries (every row) or labels_hist.
//               At the end the workgroup flushes its non-zero counters once with 64-bit integer atomics.
// Integer arithmetic only, no float atomics; a workgroup's 32-bit counters cannot overflow (nnz < 2^31, n < 2^31).  No
// workgroup waits for another.  Integer sums do not depend on the order of arrival: results are identical from call to call.
#include "cgcn_common.hpp"

#define LS_NT 256                 // threads of every kernel here
#define LS_WAVES (LS_NT / WAVE)
#define LS_AT 32                  // row labels (a) per slab tile
#define LS_ROWS 64                // rows per chunk of k_ls_pass
#define LS_LONG 256               // a row with more entries is split over the workgroup's waves
#define LS_MAX_C 256               // CGCN_LABELSTATS_MAX_C: W = (C + 63) / 64 <= 4

typedef unsigned long long u64;

// bits[u * W + w] bit l  <=>  targets[u, 64 w + l] != 0
__global__ __launch_bounds__(LS_NT) void k_ls_pack(int n, int C, int W, const float* __restrict__ targets,
                                                   u64* __restrict__ bits) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long long items = (long long)n * W;
  for (long long it = (long long)blockIdx.x * LS_WAVES + threadIdx.x / WAVE; it < items; it += (long long)gridDim.x * LS_WAVES) {
    const long long u = it / W;
    const int c = (int)(it % W) * 64 + lane;
    const bool pos = c < C && targets[(size_t)u * C + c] != 0.f;
    const u64 m = __ballot(pos);
    if (lane == 0) bits[it] = m;
  }
}

// Tile blockIdx.y holds the row labels a0 .. a0 + LS_AT - 1, a0 = LS_AT * blockIdx.y.  Dynamic LDS, 32-bit words:
//   slab[LS_AT][64 W] pair counters, dsum[LS_AT] degree counters, then (tile 0) hist[C + 1] (window pass) or ent[1] (graph pass).
// out_pairs: cooccurrence / contact_pairs [C, C]; out_sum: label_count / degree_sum [C]; out_extra: labels_hist [C + 1] /
// n_entries [1].
template <bool GRAPH, int W>
__global__ __launch_bounds__(LS_NT) void k_ls_pass(int n, int C, long long nnz, const int* __restrict__ rowptr,
                                                   const int* __restrict__ col, const float* __restrict__ val,
                                                   const u64* __restrict__ bits, u64* __restrict__ out_pairs,
                                                   u64* __restrict__ out_sum, u64* __restrict__ out_extra) {
  extern __shared__ __attribute__((aligned(16))) unsigned int ls_lds[];
  constexpr int CP = 64 * W;
  unsigned int* slab = ls_lds;
  unsigned int* dsum = slab + LS_AT * CP;
  unsigned int* extra = dsum + LS_AT;
  const int t = threadIdx.x, lane = t & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(t / WAVE);   // wave-uniform, and known to be
  const int tile = blockIdx.y, a0 = tile * LS_AT;
  const int n_extra = tile == 0 ? (GRAPH ? 1 : C + 1) : 0;
  const int words = LS_AT * CP + LS_AT + n_extra;
  for (int i = t; i < words; i += LS_NT) ls_lds[i] = 0u;
  __syncthreads();

  const int aw = a0 >> 6, ash = a0 & 63;   // the tile's labels are bits ash .. ash + 31 of word aw
  for (long long r0 = (long long)blockIdx.x * LS_ROWS; r0 < n; r0 += (long long)gridDim.x * LS_ROWS) {
    const int r1 = (int)min((long long)n, r0 + LS_ROWS);
    for (int u = (int)r0; u < r1; ++u) {
      unsigned int amask = (unsigned int)(bits[(size_t)u * W + aw] >> ash);
      unsigned int nb[W];
      unsigned int deg = 0;
      if (!GRAPH) {
        if ((u & (LS_WAVES - 1)) != wv) continue;
        int k = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) {
          const u64 m = bits[(size_t)u * W + w];
          nb[w] = (unsigned int)(m >> lane) & 1u;
          k += __popcll(m);
        }
        deg = 1;
        if (tile == 0 && lane == 0) atomicAdd(&extra[k], 1u);
      } else {
        if (amask == 0u && tile != 0) continue;   // nothing of this row lands in the tile (tile 0 still counts its entries)
        long long p0 = rowptr[u], p1 = rowptr[u + 1];
        p0 = p0 < 0 ? 0 : p0;
        p1 = p1 > nnz ? nnz : p1;                 // a corrupt rowptr never reads past the arrays
        const bool split = p1 - p0 > LS_LONG;
        if (!split && (u & (LS_WAVES - 1)) != wv) continue;
#pragma unroll
        for (int w = 0; w < W; ++w) nb[w] = 0u;
        const long long step = split ? LS_WAVES * WAVE : WAVE;
        for (long long base = p0 + (split ? wv * WAVE : 0); base < p1; base += step) {
          const long long p = base + lane;
          int v = -1;
          if (p < p1) {
            v = col[p];
            if (v == u || (unsigned int)v >= (unsigned int)n || (val && !(val[p] > 0.f))) v = -1;   // not a neighbour entry
          }
          const u64 live = __ballot(v >= 0);
          deg += (unsigned int)__popcll(live);
          if (amask == 0u || live == 0ull) continue;
          u64 mine[W];
#pragma unroll
          for (int w = 0; w < W; ++w) mine[w] = v >= 0 ? bits[(size_t)v * W + w] : 0ull;
          const int cnt = (int)min((long long)WAVE, p1 - base);
          for (int j = 0; j < cnt; ++j) {
#pragma unroll
            for (int w = 0; w < W; ++w) {
              const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)mine[w], j);
              const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(mine[w] >> 32), j);
              const u64 m = ((u64)hi << 32) | lo;
              nb[w] += (unsigned int)(m >> lane) & 1u;
            }
          }
        }
        if (tile == 0 && lane == 0 && deg) atomicAdd(&extra[0], deg);
      }
      // add nb into row a of the slab, and deg to a's degree counter, for every label a of the tile that the row carries
      while (amask) {
        const int a = __ffs(amask) - 1;
        amask &= amask - 1u;
#pragma unroll
        for (int w = 0; w < W; ++w)
          if (nb[w]) atomicAdd(&slab[a * CP + w * 64 + lane], nb[w]);
        if (lane == 0 && deg) atomicAdd(&dsum[a], deg);
      }
    }
  }
  __syncthreads();

  // one flush per workgroup: non-zero counters only, 64-bit integer atomics
  for (int i = t; i < LS_AT * CP; i += LS_NT) {
    const unsigned int c = slab[i];
    const int a = a0 + i / CP, b = i % CP;
    if (c && a < C && b < C) atomicAdd(&out_pairs[(size_t)a * C + b], (u64)c);
  }
  if (t < LS_AT && a0 + t < C && dsum[t]) atomicAdd(&out_sum[a0 + t], (u64)dsum[t]);
  for (int i = t; i < n_extra; i += LS_NT)
    if (extra[i]) atomicAdd(&out_extra[i], (u64)extra[i]);
}

static inline size_t ls_align(size_t b) { return (b + 255) & ~(size_t)255; }
static inline bool ls_c_ok(int C) { return C >= 1 && C <= LS_MAX_C; }
static inline size_t ls_bits_bytes(int n, int C) { return ls_align((size_t)(n > 0 ? n : 1) * ((C + 63) / 64) * sizeof(u64)); }

template <bool GRAPH>
static void ls_launch(hipStream_t st, int n, int C, long long nnz, const int* rowptr, const int* col, const float* val,
                      const u64* bits, u64* out_pairs, u64* out_sum, u64* out_extra) {
  const int W = (C + 63) / 64, tiles = (C + LS_AT - 1) / LS_AT;
  const int chunks = (n + LS_ROWS - 1) / LS_ROWS;
  const int cap = 2048 / tiles;
  const dim3 grid(chunks < cap ? chunks : cap, tiles);
  const size_t lds = ((size_t)LS_AT * 64 * W + LS_AT + (GRAPH ? 1 : C + 1)) * sizeof(unsigned int);
#define LS_GO(WW)                                                                                                          \
  hipLaunchKernelGGL((k_ls_pass<GRAPH, WW>), grid, dim3(LS_NT), lds, st, n, C, nnz, rowptr, col, val, bits, out_pairs, out_sum, \
                     out_extra)
  switch (W) {
    case 1: LS_GO(1); break;
    case 2: LS_GO(2); break;
    case 3: LS_GO(3); break;
    default: LS_GO(4); break;
  }
#undef LS_GO
}

extern "C" {

size_t cgcn_labelstats_workspace_bytes(int n, int C) {
  if (n < 0 || !ls_c_ok(C)) return 0;
  return ls_bits_bytes(n, C);
}

int cgcn_labelstats_windows(cgcn_stream_t stream, int n, int C, const float* targets, void* workspace, size_t workspace_bytes,
                            long long* label_count, long long* labels_hist, long long* cooccurrence, int accumulate) {
  if (!ls_c_ok(C)) return CGCN_ERR_UNSUPPORTED;
  if (n < 0) return CGCN_ERR_BAD_ARG;
  if (!label_count || !labels_hist || !cooccurrence || (n > 0 && (!targets || !workspace))) return CGCN_ERR_BAD_ARG;
  if (n > 0 && workspace_bytes < ls_bits_bytes(n, C)) return CGCN_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (!accumulate) {
    if (hipMemsetAsync(label_count, 0, (size_t)C * sizeof(long long), st) != hipSuccess ||
        hipMemsetAsync(labels_hist, 0, (size_t)(C + 1) * sizeof(long long), st) != hipSuccess ||
        hipMemsetAsync(cooccurrence, 0, (size_t)C * C * sizeof(long long), st) != hipSuccess)
      return CGCN_ERR_LAUNCH;
  }
  if (n == 0) return CGCN_OK;
  const int W = (C + 63) / 64;
  const long long waves = (long long)n * W;
  const long long blocks = (waves + LS_WAVES - 1) / LS_WAVES;
  hipLaunchKernelGGL(k_ls_pack, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(LS_NT), 0, st, n, C, W, targets,
                     (u64*)workspace);
  ls_launch<false>(st, n, C, 0, nullptr, nullptr, nullptr, (const u64*)workspace, (u64*)cooccurrence, (u64*)label_count,
                   (u64*)labels_hist);
  return launch_status();
}

int cgcn_labelstats_graph(cgcn_stream_t stream, int n, int C, long long nnz, const int32_t* rowptr, const int32_t* col,
                          const float* val, const void* label_bits, size_t label_bits_bytes, long long* degree_sum,
                          long long* contact_pairs, long long* n_entries, int accumulate) {
  if (!ls_c_ok(C) || nnz >= (1ll << 31)) return CGCN_ERR_UNSUPPORTED;
  if (n < 0 || nnz < 0) return CGCN_ERR_BAD_ARG;
  if (!degree_sum || !contact_pairs || !n_entries || (n > 0 && (!rowptr || !label_bits)) || (nnz > 0 && !col))
    return CGCN_ERR_BAD_ARG;
  if (n > 0 && label_bits_bytes < ls_bits_bytes(n, C)) return CGCN_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (!accumulate) {
    if (hipMemsetAsync(degree_sum, 0, (size_t)C * sizeof(long long), st) != hipSuccess ||
        hipMemsetAsync(contact_pairs, 0, (size_t)C * C * sizeof(long long), st) != hipSuccess ||
        hipMemsetAsync(n_entries, 0, sizeof(long long), st) != hipSuccess)
      return CGCN_ERR_LAUNCH;
  }
  if (n == 0 || nnz == 0) return CGCN_OK;
  ls_launch<true>(st, n, C, nnz, rowptr, col, val, (const u64*)label_bits, (u64*)contact_pairs, (u64*)degree_sum,
                  (u64*)n_entries);
  return launch_status();
}

}  // extern "C"
