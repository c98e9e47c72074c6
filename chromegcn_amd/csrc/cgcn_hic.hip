// chromegcn_amd/csrc/cgcn_hic.hip
//
// The top-K Hi-C contact graph from raw contact records on the device: what the reference's
// data/7create_graph_new.py does with a Python dict and a full sorted() -- get_contact_edge_pairs (:67-91),
// get_top_contact_locs (:93-104), create_adj_mat (:108-120) -- for any edge budget and any normalisation vector.
//
//   k_hic_filter<false>  one streaming pass over the M records (pos1, pos2 only): survivors per 2048-record tile
//   k_tile_scan          exclusive scan of the tile counts (one workgroup); the survivor count S stays on the device
//   k_hic_filter<true>   the same pass again, now writing the survivors IN FILE ORDER: the sort key of the fp64 value
//                        count / (nv[pos1 / res] * nv[pos2 / res]) and its window ranks (i, j)
//   rocprim::radix_sort_keys    a copy of the keys, ascending (= values descending)
//   k_hic_threshold      t = the K-th sorted key and how many survivors with key t are taken: K - #{keys < t}
//   k_hic_take<false> / k_tile_scan / k_hic_take<true>  a survivor is taken iff key < t, or key == t and fewer than that many
//                        survivors with key t precede it IN FILE ORDER (an ordered prefix count): the reference's stable
//                        sorted(reverse=True) cut at K, without ordering the survivors; the taken ones leave as edge keys
//                        (i << b | j) and (j << b | i), b = bits of N, the others as padding
//   rocprim::radix_sort_keys    the 2 b low bits of the edge keys (the padding sorts last)
//   k_hic_unique<false> / k_tile_scan / k_hic_unique<true>   duplicates dropped ((a, b) and (b, a) records merge), columns,
//                        row pointers and nnz
// Integer keys, integer counts and ordered writes only: the result does not depend on scheduling.  Nothing is allocated,
// nothing synchronises, nothing is retained; every size the host cannot know (S, min(K, S), nnz) is read from device
// memory by the kernels, whose grids are sized for the caller's bounds (capacity, K).
#include <cstring>  // rocprim 4.x headers use memset without including it
#include <rocprim/rocprim.hpp>

#include "cgcn_compact.hpp"
#include "cgcn_hicmap.hpp"

#define HIC_THREADS 256
#define HIC_STEPS 8                                    // records per lane of the filter pass
#define HIC_TILE (HIC_THREADS * HIC_STEPS)             // records per workgroup: 4 waves x 8 steps x 64 lanes
#define HIC_PAD_KEY 0xFFFFFFFFFFFFFFFFull              // sorts behind every real key in both sorts

// rank of x in the strictly increasing ws[0..N), or -1.  Branch-free descent to the last element <= x.
__device__ __forceinline__ int hic_rank(const int* __restrict__ ws, int N, int x) {
  int lo = 0, n = N;
  while (n > 1) {
    const int half = n >> 1;
    lo = ws[lo + half] <= x ? lo + half : lo;
    n -= half;
  }
  return (N > 0 && ws[lo] == x) ? lo : -1;
}

// The order-preserving image of an fp64 value, complemented: an ASCENDING sort of these keys lists the values in
// descending order.  -0 is folded onto +0 (the reference compares numbers).
__device__ __forceinline__ u64 hic_value_key(double v) {
  u64 u = (u64)__double_as_longlong(v == 0.0 ? 0.0 : v);
  u ^= (u >> 63) ? 0xFFFFFFFFFFFFFFFFull : 0x8000000000000000ull;
  return ~u;
}

// nv[] of get_normalization_values (:62-63): NaN and 0 become +inf.  A bin outside the vector (the reference raises
// IndexError) reads as +inf too: never out of bounds.
__device__ __forceinline__ double hic_norm_at(const double* __restrict__ norm, long long n_bins, int pos, int res) {
  return hm_norm_at(norm, n_bins, pos / res);
}

// Distance-aware variants (DIST = true in the filter passes below): a record takes part only if
// |pos1 - pos2| >= min_d (in 64 bits), and its value is divided once more, by ex[d], d = |pos1 // res - pos2 // res|.
// ex[] as nv[]: NaN, 0 and negative entries read as +inf, and so does a distance outside the vector: never out of bounds.
__device__ __forceinline__ bool hic_gap_ok(int a, int b, long long min_d) {
  const long long g = (long long)a - (long long)b;
  return (g < 0 ? -g : g) >= min_d;
}
__device__ __forceinline__ long long hic_floor_bin(int pos, int res) {   // numpy's pos // res
  const long long q = pos / res;
  return (pos < 0 && q * res != pos) ? q - 1 : q;
}
__device__ __forceinline__ double hic_expected_at(const double* __restrict__ ex, long long n_ex, int p1, int p2, int res) {
  const long long g = hic_floor_bin(p1, res) - hic_floor_bin(p2, res), d = g < 0 ? -g : g;
  if (d >= n_ex) return hm_inf();
  const double x = ex[d];
  return x > 0.0 ? x : hm_inf();
}

// Wave w of a workgroup owns the 512 consecutive records [tile + 512 w, tile + 512 (w + 1)) and walks them in 8 steps of
// 64 (coalesced); a survivor's place is (tile offset) + (survivors of the waves before) + (of the steps before) + (of the
// lanes before): file order.  WRITE = false only counts the tile's survivors.
template <bool WRITE, bool DIST>
__device__ __forceinline__ void hic_filter_body(long long M, const int* __restrict__ pos1, const int* __restrict__ pos2,
                                                const double* __restrict__ count, const double* __restrict__ norm,
                                                long long n_bins, int res, const int* __restrict__ ws, int N,
                                                int* __restrict__ tile_counts, const long long* __restrict__ tile_off,
                                                long long capacity, u64* __restrict__ keys, int2* __restrict__ ij, long long min_d,
                                                const double* __restrict__ ex, long long n_ex) {
  __shared__ int wave_tot[HIC_THREADS / WAVE];
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  const long long base = (long long)blockIdx.x * HIC_TILE + (long long)w * (HIC_STEPS * WAVE);
  int ri[HIC_STEPS], rj[HIC_STEPS];
  int before[HIC_STEPS];   // survivors of this wave in earlier steps and earlier lanes of the step
  int run = 0;
#pragma unroll
  for (int s = 0; s < HIC_STEPS; ++s) {
    const long long r = base + s * WAVE + lane;
    int i = -1, j = -1;
    if (r < M) {
      const int a = pos1[r], b = pos2[r];
      if (a != b && (!DIST || hic_gap_ok(a, b, min_d))) {
        i = hic_rank(ws, N, a);
        if (i >= 0) j = hic_rank(ws, N, b);
      }
    }
    const bool hit = i >= 0 && j >= 0;
    const u64 m = __ballot(hit);
    before[s] = run + __popcll(m & ((1ull << lane) - 1ull));
    run += __popcll(m);
    ri[s] = hit ? i : -1;
    rj[s] = j;
  }
  if (lane == 0) wave_tot[w] = run;
  __syncthreads();
  if (!WRITE) {
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
    return;
  }
  long long off = tile_off[blockIdx.x];
  for (int k = 0; k < w; ++k) off += wave_tot[k];
#pragma unroll
  for (int s = 0; s < HIC_STEPS; ++s) {
    if (ri[s] < 0) continue;
    const long long o = off + before[s];
    if (o >= capacity) continue;   // the caller's capacity is below the survivor count: the build reports it, nothing is overrun
    const long long r = base + s * WAVE + lane;
    double v = count[r];
    if (norm) {
      const double d = hic_norm_at(norm, n_bins, pos1[r], res) * hic_norm_at(norm, n_bins, pos2[r], res);
      v = v / d;   // one multiply, one divide, both correctly rounded (:84)
    }
    if (DIST && ex) v = v / hic_expected_at(ex, n_ex, pos1[r], pos2[r], res);   // observed / expected: a second division
    keys[o] = hic_value_key(v);
    ij[o] = make_int2(ri[s], rj[s]);
  }
}

template <bool WRITE>
__global__ __launch_bounds__(HIC_THREADS) void k_hic_filter(long long M, const int* __restrict__ pos1, const int* __restrict__ pos2,
                                                            const double* __restrict__ count, const double* __restrict__ norm,
                                                            long long n_bins, int res, const int* __restrict__ ws, int N,
                                                            int* __restrict__ tile_counts, const long long* __restrict__ tile_off,
                                                            long long capacity, u64* __restrict__ keys, int2* __restrict__ ij) {
  hic_filter_body<WRITE, false>(M, pos1, pos2, count, norm, n_bins, res, ws, N, tile_counts, tile_off, capacity, keys, ij, 0ll, nullptr,
                                0ll);
}

// ... with the minimum gap and the expected vector (ex may be NULL: the gap alone)
template <bool WRITE>
__global__ __launch_bounds__(HIC_THREADS) void k_hic_filter_dist(long long M, const int* __restrict__ pos1, const int* __restrict__ pos2,
                                                                 const double* __restrict__ count, const double* __restrict__ norm,
                                                                 long long n_bins, int res, const int* __restrict__ ws, int N,
                                                                 int* __restrict__ tile_counts, const long long* __restrict__ tile_off,
                                                                 long long capacity, u64* __restrict__ keys, int2* __restrict__ ij,
                                                                 long long min_d, const double* __restrict__ ex, long long n_ex) {
  hic_filter_body<WRITE, true>(M, pos1, pos2, count, norm, n_bins, res, ws, N, tile_counts, tile_off, capacity, keys, ij, min_d, ex,
                               n_ex);
}

// slots [S, capacity) of the sort input, when the caller's capacity exceeds the survivor count
__global__ __launch_bounds__(256) void k_hic_pad(const long long* __restrict__ n_surv, long long capacity, u64* __restrict__ keys) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o < capacity && o >= n_surv[0]) keys[o] = HIC_PAD_KEY;
}

// From the sorted keys: taken[0] = kt = min(K, S, capacity); thr[0] = t, the kt-th key (the K-th largest value);
// thr[1] = kt - #{keys < t}, the number of survivors with value == t that are taken (the first ones in file order).
// kt = 0: t = 0 and nothing is below it.  One thread; the count is a binary search.
__global__ void k_hic_threshold(long long K, long long capacity, const long long* __restrict__ n_surv, const u64* __restrict__ sorted,
                                long long* __restrict__ taken, u64* __restrict__ thr) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const long long S = min(n_surv[0], capacity);
  const long long kt = min(K, S);
  taken[0] = kt;
  if (kt == 0) { thr[0] = 0; thr[1] = 0; return; }
  const u64 t = sorted[kt - 1];
  long long lo = 0, hi = kt - 1;   // first index with sorted[index] == t
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (sorted[mid] < t) lo = mid + 1; else hi = mid;
  }
  thr[0] = t;
  thr[1] = (u64)(kt - lo);
}

// Survivor o (file order) is taken iff its key is below t (its value above the threshold) or equals t and fewer than thr[1]
// survivors with key t precede it.  WRITE = false counts the keys equal to t per 256-survivor tile; WRITE = true writes the
// two edge keys of every taken survivor at slots 2 o and 2 o + 1 and pads the others (the edge sort moves the pads behind).
template <bool WRITE>
__global__ __launch_bounds__(256) void k_hic_take(const long long* __restrict__ n_surv, long long capacity, const u64* __restrict__ keys,
                                                  const u64* __restrict__ thr, int* __restrict__ tile_counts,
                                                  const long long* __restrict__ tile_off, const int2* __restrict__ ij, int b,
                                                  u64* __restrict__ edges) {
  __shared__ int wave_tot[4];
  const long long S = min(n_surv[0], capacity);
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  const u64 t = thr[0];
  const u64 key = o < S ? keys[o] : HIC_PAD_KEY;
  const bool eq = o < S && key == t;
  const WgFlags<> eqs(eq, wave_tot);
  if (!WRITE) {
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = eqs.count();
    return;
  }
  if (o >= capacity) return;
  const long long rank = eqs.before(tile_off[blockIdx.x]);
  u64 e0 = HIC_PAD_KEY, e1 = HIC_PAD_KEY;
  if (o < S && (key < t || (eq && (u64)rank < thr[1]))) {
    const int2 p = ij[o];
    e0 = ((u64)(unsigned)p.x << b) | (u64)(unsigned)p.y;
    e1 = ((u64)(unsigned)p.y << b) | (u64)(unsigned)p.x;
  }
  edges[2 * o] = e0;
  edges[2 * o + 1] = e1;
}

// sorted edge keys [0, 2 taken): element p starts a new (row, column) pair iff it differs from p - 1.  WRITE = false counts
// the starts per 256-element tile; WRITE = true writes the columns and the row pointers: the start at output place q of
// row i closes every row after the previous pair's up to i (rowptr[r] = q), the last element closes the rest with nnz.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_hic_unique(const long long* __restrict__ taken, const u64* __restrict__ edges, int b, int N,
                                                    int* __restrict__ tile_counts, const long long* __restrict__ tile_off,
                                                    const int* __restrict__ nnz, int* __restrict__ rowptr, int* __restrict__ col) {
  __shared__ int wave_tot[4];
  const long long n = 2 * taken[0];
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  u64 e = 0, prev = 0;
  bool head = false;
  if (p < n) {
    e = edges[p];
    prev = p > 0 ? edges[p - 1] : 0;
    head = p == 0 || e != prev;
  }
  const WgFlags<> heads(head, wave_tot);
  if (!WRITE) {
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = heads.count();
    return;
  }
  if (p >= n) return;
  const int row = (int)(e >> b);
  if (head) {
    const long long q = heads.before(tile_off[blockIdx.x]);
    col[q] = (int)(e & ((1ull << b) - 1ull));
    const int prow = p > 0 ? (int)(prev >> b) : -1;
    for (int r = prow + 1; r <= row; ++r) rowptr[r] = (int)q;
  }
  if (p == n - 1) {
    const int total = nnz[0];
    for (int r = row + 1; r <= N; ++r) rowptr[r] = total;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Records coarser than the windows (K562: 5 kb records, 1 kb windows).  up = resolution_bp /
// window_bp; a record stands for its up x up children (pos1 + a window_bp, pos2 + b window_bp), a outer, b inner, and the
// rule above applies to that expanded file.  Nothing is expanded in memory: the filter reads the 16 B of a source record and
// writes only the surviving children, at their places in the expanded file's survivor order.
//
//   k_hic_up_bits / k_hic_up_rank   once per call: a bitmap with one bit per window_bp bin and, per 32-bit word, the number
//                        of windows before it.  A window start that is negative or no multiple of window_bp raises a flag
//                        instead: the passes then find every child by binary search (the rule, for any window set).
//   k_hic_filter_up<false>  per record the two up-bit masks m1, m2 of its children that are windows (one two-word table
//                        read each); it has popc(m1) popc(m2) - (pos1 == pos2 ? popc(m1 & m2) : 0) survivors.  A wave owns
//                        512 consecutive records and walks them in 8 steps of 64; the counts are scanned across the wave
//                        with DPP row shifts.  One count per 512-record wave tile: no barrier between the waves.
//   k_tile_scan          as above, over the wave tiles
//   k_hic_filter_up<true>   the same pass, writing: the value key once per record, (i, j) from the rank table
// The workgroups are persistent (a wave strides over the wave tiles) so that the copy of the tables into LDS -- up to
// 2 x 32 KB -- is paid once per workgroup; larger tables are read from global memory (L2) by the same code.
#define HIC_UP_THREADS 1024
#define HIC_UP_WAVES (HIC_UP_THREADS / WAVE)
#define HIC_UP_WTILE (HIC_STEPS * WAVE)                // records per wave tile
#define HIC_UP_MAX 8
#define HIC_UP_LDS_WORDS 8192                          // bitmap words (and rank words) that the LDS route holds

__global__ __launch_bounds__(256) void k_hic_up_bits(const int* __restrict__ ws, int N, int wbp, long long nbits,
                                                     unsigned* __restrict__ bitmap, int* __restrict__ offgrid) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int s = ws[i];
  if (s < 0 || s % wbp != 0) { atomicOr(offgrid, 1); return; }
  const long long q = s / wbp;
  if (q < nbits) atomicOr(&bitmap[q >> 5], 1u << (q & 31));   // a start beyond the caller's extent is ignored
}

// rank[w] = set bits of bitmap[0..w).  One workgroup of 1024 threads (the skeleton of k_tile_scan, cgcn_compact.hpp).
__global__ __launch_bounds__(1024) void k_hic_up_rank(int nwords, const unsigned* __restrict__ bitmap, int* __restrict__ rank) {
  __shared__ int part[1024];
  const int t = threadIdx.x;
  const int per = (nwords + 1023) / 1024;
  const int i0 = min(nwords, t * per), i1 = min(nwords, i0 + per);
  int s = 0;
  for (int i = i0; i < i1; ++i) s += __popc(bitmap[i]);
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = t ? part[t - 1] : 0;
  for (int i = i0; i < i1; ++i) {
    rank[i] = run;
    run += __popc(bitmap[i]);
  }
}

// inclusive sum over the 64 lanes of a wave (every lane active): 4 row shifts inside the rows of 16, then the two row
// broadcasts.  A lane without a source keeps the 0 of `old`.
__device__ __forceinline__ int hic_wave_scan(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);   // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);   // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);   // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);   // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);   // row_bcast:15 into rows 1 and 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);   // row_bcast:31 into rows 2 and 3
  return v;
}

// which of the children pos + a window_bp, a < up, are windows: bit a.  Bitmap route (every window start is a non-negative
// multiple of window_bp): bits [q, q + up) of the bitmap, q = pos / window_bp; the bitmap ends with a zero word, so the
// second word of the read exists.  Search route: the rule, child by child.
__device__ __forceinline__ unsigned hic_up_mask(bool search, const unsigned* bm, long long nbits, int wbp, int up, int pos,
                                                const int* __restrict__ ws, int N) {
  const unsigned all = (1u << up) - 1u;
  if (search) {
    unsigned m = 0;
    for (int a = 0; a < up; ++a) {
      const long long c = (long long)pos + (long long)a * wbp;
      if (c <= 2147483647ll && (c < 0 || c / wbp < nbits) && hic_rank(ws, N, (int)c) >= 0) m |= 1u << a;
    }
    return m;
  }
  const long long q = pos / wbp;
  if (q * wbp != pos || q >= nbits || q <= -(long long)up) return 0;
  if (q < 0) return (bm[0] << (unsigned)(-q)) & all;
  const unsigned w = (unsigned)(q >> 5);
  const u64 two = (u64)bm[w] | ((u64)bm[w + 1] << 32);
  return (unsigned)(two >> (q & 31)) & all;
}

// windows before bin q >= 0 (bitmap route)
__device__ __forceinline__ int hic_up_rank_of(const unsigned* bm, const int* rk, long long q) {
  const unsigned w = (unsigned)(q >> 5);
  return rk[w] + __popc(bm[w] & ((1u << (q & 31)) - 1u));
}

template <bool WRITE, bool LDS, bool DIST>
__device__ __forceinline__ void hic_filter_up_body(
    long long M, const int* __restrict__ pos1, const int* __restrict__ pos2, const double* __restrict__ count,
    const double* __restrict__ norm, long long n_bins, int res, int wbp, int up, const int* __restrict__ ws, int N,
    const unsigned* __restrict__ tab, int nwords, long long nbits, const int* __restrict__ offgrid, long long wtiles,
    int* __restrict__ tile_counts, const long long* __restrict__ tile_off, long long capacity, u64* __restrict__ keys,
    int2* __restrict__ ij, long long min_d, const double* __restrict__ ex, long long n_ex) {
  extern __shared__ unsigned hic_up_lds[];
  const bool search = offgrid[0] != 0;
  const unsigned* bm = tab;
  if (LDS) {
    if (!search)
      for (int k = threadIdx.x; k < 2 * nwords; k += HIC_UP_THREADS) hic_up_lds[k] = tab[k];
    __syncthreads();
    bm = hic_up_lds;
  }
  const int* rk = (const int*)(bm + nwords);
  const int lane = threadIdx.x & (WAVE - 1);
  const long long wave0 = (long long)blockIdx.x * HIC_UP_WAVES + threadIdx.x / WAVE, waves = (long long)gridDim.x * HIC_UP_WAVES;
  for (long long t = wave0; t < wtiles; t += waves) {
    const long long base = t * HIC_UP_WTILE;
    unsigned pk[HIC_STEPS];   // m1 | m2 << 8 | (pos1 == pos2) << 16; 0 = no survivor
    int before[HIC_STEPS];    // survivors of this wave tile in earlier steps and earlier lanes of the step
    int run = 0;
#pragma unroll
    for (int s = 0; s < HIC_STEPS; ++s) {
      const long long r = base + s * WAVE + lane;
      unsigned m1 = 0, m2 = 0, diag = 0;
      if (r < M) {
        const int a = pos1[r], b = pos2[r];
        if (!DIST || hic_gap_ok(a, b, min_d)) m1 = hic_up_mask(search, bm, nbits, wbp, up, a, ws, N);   // the SOURCE record's gap
        if (m1) m2 = hic_up_mask(search, bm, nbits, wbp, up, b, ws, N);
        diag = a == b;
      }
      const int cnt = __popc(m1) * __popc(m2) - (diag ? __popc(m1 & m2) : 0);
      const int inc = hic_wave_scan(cnt);
      before[s] = run + inc - cnt;
      run += __builtin_amdgcn_readlane(inc, WAVE - 1);
      pk[s] = cnt > 0 ? (m1 | (m2 << 8) | (diag << 16)) : 0u;
    }
    if (!WRITE) {
      if (lane == 0) tile_counts[t] = run;
      continue;
    }
    const long long off = tile_off[t];
#pragma unroll
    for (int s = 0; s < HIC_STEPS; ++s) {
      if (pk[s] == 0) continue;
      long long o = off + before[s];
      if (o >= capacity) continue;   // the caller's capacity is below the survivor count: the build reports it, nothing is overrun
      const long long r = base + s * WAVE + lane;
      const int p1 = pos1[r], p2 = pos2[r];
      double v = count[r];
      if (norm) {
        const double d = hic_norm_at(norm, n_bins, p1, res) * hic_norm_at(norm, n_bins, p2, res);
        v = v / d;   // one multiply, one divide: every child of the record has the record's two norm bins
      }
      if (DIST && ex) v = v / hic_expected_at(ex, n_ex, p1, p2, res);   // ... and the record's distance
      const u64 key = hic_value_key(v);
      const unsigned m1 = pk[s] & 0xFFu, m2 = (pk[s] >> 8) & 0xFFu;
      const bool diag = (pk[s] >> 16) != 0;
      int ibase = 0, jbase = 0;
      if (!search) {   // m1, m2 != 0; a set bit is a bin >= 0
        ibase = hic_up_rank_of(bm, rk, p1 / wbp + (__ffs(m1) - 1));
        jbase = hic_up_rank_of(bm, rk, p2 / wbp + (__ffs(m2) - 1));
      }
      for (unsigned ma = m1; ma; ma &= ma - 1u) {
        const int a = __ffs(ma) - 1;
        const int i = search ? hic_rank(ws, N, p1 + a * wbp) : ibase + __popc(m1 & ((1u << a) - 1u));
        for (unsigned mb = m2; mb; mb &= mb - 1u) {
          const int b = __ffs(mb) - 1;
          if (diag && a == b) continue;
          if (o >= capacity) break;
          const int j = search ? hic_rank(ws, N, p2 + b * wbp) : jbase + __popc(m2 & ((1u << b) - 1u));
          keys[o] = key;
          ij[o] = make_int2(i, j);
          ++o;
        }
      }
    }
  }
}

template <bool WRITE, bool LDS>
__global__ __launch_bounds__(HIC_UP_THREADS) void k_hic_filter_up(
    long long M, const int* __restrict__ pos1, const int* __restrict__ pos2, const double* __restrict__ count,
    const double* __restrict__ norm, long long n_bins, int res, int wbp, int up, const int* __restrict__ ws, int N,
    const unsigned* __restrict__ tab, int nwords, long long nbits, const int* __restrict__ offgrid, long long wtiles,
    int* __restrict__ tile_counts, const long long* __restrict__ tile_off, long long capacity, u64* __restrict__ keys,
    int2* __restrict__ ij) {
  hic_filter_up_body<WRITE, LDS, false>(M, pos1, pos2, count, norm, n_bins, res, wbp, up, ws, N, tab, nwords, nbits, offgrid, wtiles,
                                        tile_counts, tile_off, capacity, keys, ij, 0ll, nullptr, 0ll);
}

template <bool WRITE, bool LDS>
__global__ __launch_bounds__(HIC_UP_THREADS) void k_hic_filter_up_dist(
    long long M, const int* __restrict__ pos1, const int* __restrict__ pos2, const double* __restrict__ count,
    const double* __restrict__ norm, long long n_bins, int res, int wbp, int up, const int* __restrict__ ws, int N,
    const unsigned* __restrict__ tab, int nwords, long long nbits, const int* __restrict__ offgrid, long long wtiles,
    int* __restrict__ tile_counts, const long long* __restrict__ tile_off, long long capacity, u64* __restrict__ keys,
    int2* __restrict__ ij, long long min_d, const double* __restrict__ ex, long long n_ex) {
  hic_filter_up_body<WRITE, LDS, true>(M, pos1, pos2, count, norm, n_bins, res, wbp, up, ws, N, tab, nwords, nbits, offgrid, wtiles,
                                       tile_counts, tile_off, capacity, keys, ij, min_d, ex, n_ex);
}

struct HicPlan {
  long long cap, half, E;      // survivor slots, the most records taken = min(K, capacity), edge slots = 2 cap
  long long tilesM, tilesS, tilesE;
  int b;
  size_t temp, o_counts, o_off, o_taken, o_thr, o_keyA, o_keyB, o_ij, o_edgeA, o_edgeB, o_temp, total;
};

static bool hic_plan(long long M, int N, long long capacity, long long K, HicPlan* p) {
  if (M < 0 || N < 0 || capacity < 0 || K < 0) return false;
  if (capacity >= 2147483647ll || 2 * K >= 2147483648ll || M / HIC_TILE >= 2147483647ll) return false;
  p->cap = capacity < 1 ? 1 : capacity;
  p->half = K < capacity ? K : capacity;
  p->E = 2 * p->cap;
  p->tilesM = tiles_of(M, HIC_TILE);
  p->tilesS = tiles_of(p->cap, 256);
  p->tilesE = tiles_of(p->E, 256);
  p->b = bits_for(N);
  size_t t1 = 0, t2 = 0;
  (void)rocprim::radix_sort_keys(nullptr, t1, (const u64*)nullptr, (u64*)nullptr, (size_t)p->cap, 0u, 64u);
  (void)rocprim::radix_sort_keys(nullptr, t2, (const u64*)nullptr, (u64*)nullptr, (size_t)p->E, 0u, (unsigned)(2 * p->b));
  p->temp = t1 > t2 ? t1 : t2;
  const long long tiles = p->tilesM > p->tilesE ? p->tilesM : p->tilesE;
  const size_t e = (size_t)p->E;
  WsBump w = {0};
  p->o_counts = w.take((size_t)tiles * 4);
  p->o_off = w.take((size_t)tiles * 8);
  p->o_taken = w.take(256);
  p->o_thr = w.take(256);
  p->o_keyA = w.take((size_t)p->cap * 8);
  p->o_keyB = w.take((size_t)p->cap * 8);
  p->o_ij = w.take((size_t)p->cap * 8);
  p->o_edgeA = w.take(e * 8);
  p->o_edgeB = w.take(e * 8);
  p->o_temp = w.take(p->temp);
  p->total = w.o + 256;   // the base is rounded up to 256 bytes
  return true;
}


// everything behind the filter: survivors [0, min(S, capacity)) of keyA / ij -> the CSR
static int hic_select_and_csr(hipStream_t st, const HicPlan& p, char* w, int N, long long K, long long capacity, int32_t* rowptr_out,
                              int32_t* col_out, int32_t* nnz_out, long long* n_survivors) {
  int* counts = (int*)(w + p.o_counts);
  long long* off = (long long*)(w + p.o_off);
  long long* taken = (long long*)(w + p.o_taken);
  u64* thr = (u64*)(w + p.o_thr);
  u64* keyA = (u64*)(w + p.o_keyA);
  u64* keyB = (u64*)(w + p.o_keyB);
  int2* ij = (int2*)(w + p.o_ij);
  u64* edgeA = (u64*)(w + p.o_edgeA);
  u64* edgeB = (u64*)(w + p.o_edgeB);
  size_t temp = p.temp;
  hipLaunchKernelGGL(k_hic_pad, dim3((unsigned)p.tilesS), dim3(256), 0, st, (const long long*)n_survivors, capacity, keyA);
  if (rocprim::radix_sort_keys((void*)(w + p.o_temp), temp, (const u64*)keyA, keyB, (size_t)capacity, 0u, 64u, st) != hipSuccess)
    return CGCN_ERR_LAUNCH;
  hipLaunchKernelGGL(k_hic_threshold, dim3(1), dim3(64), 0, st, K, capacity, (const long long*)n_survivors, (const u64*)keyB, taken, thr);
  hipLaunchKernelGGL(k_hic_take<false>, dim3((unsigned)p.tilesS), dim3(256), 0, st, (const long long*)n_survivors, capacity,
                     (const u64*)keyA, (const u64*)thr, counts, (const long long*)nullptr, (const int2*)nullptr, p.b, (u64*)nullptr);
  hipLaunchKernelGGL(k_tile_scan<>, dim3(1), dim3(1024), 0, st, (int)p.tilesS, (const int*)counts, off, (long long*)nullptr, (int*)nullptr, 0ll);
  hipLaunchKernelGGL(k_hic_take<true>, dim3((unsigned)p.tilesS), dim3(256), 0, st, (const long long*)n_survivors, capacity,
                     (const u64*)keyA, (const u64*)thr, (int*)nullptr, (const long long*)off, (const int2*)ij, p.b, edgeA);
  if (rocprim::radix_sort_keys((void*)(w + p.o_temp), temp, (const u64*)edgeA, edgeB, (size_t)p.E, 0u, (unsigned)(2 * p.b), st) !=
      hipSuccess)
    return CGCN_ERR_LAUNCH;
  hipLaunchKernelGGL(k_hic_unique<false>, dim3((unsigned)p.tilesE), dim3(256), 0, st, (const long long*)taken, (const u64*)edgeB, p.b, N,
                     counts, (const long long*)nullptr, (const int*)nullptr, (int*)nullptr, (int*)nullptr);
  hipLaunchKernelGGL(k_tile_scan<>, dim3(1), dim3(1024), 0, st, (int)p.tilesE, (const int*)counts, off, (long long*)nullptr, nnz_out,
                     2147483647ll);
  hipLaunchKernelGGL(k_hic_unique<true>, dim3((unsigned)p.tilesE), dim3(256), 0, st, (const long long*)taken, (const u64*)edgeB, p.b, N,
                     (int*)nullptr, (const long long*)off, (const int*)nnz_out, rowptr_out, col_out);
  return launch_status();
}

struct HicUpPlan {
  HicPlan base;
  int up, nwords;
  long long wtiles;
  bool lds;
  size_t o_wcounts, o_woff, o_tab, tab_bytes, total;
};

// CGCN_OK, or the error the entry points return for these sizes
static int hic_up_plan(long long M, int N, long long capacity, long long K, int resolution_bp, int window_bp,
                       long long n_window_bins, HicUpPlan* p) {
  if (M < 0 || N < 0 || capacity < 0 || K < 0 || n_window_bins < 0) return CGCN_ERR_BAD_ARG;
  if (resolution_bp < 1 || window_bp < 1 || resolution_bp % window_bp != 0) return CGCN_ERR_BAD_ARG;
  p->up = resolution_bp / window_bp;
  if (p->up > HIC_UP_MAX) return CGCN_ERR_UNSUPPORTED;
  if (M >= (2147483648ll + p->up * p->up - 1) / (p->up * p->up)) return CGCN_ERR_UNSUPPORTED;   // M up^2 >= 2^31
  if (n_window_bins > 2147483648ll) return CGCN_ERR_UNSUPPORTED;   // positions are int32
  if (!hic_plan(M, N, capacity, K, &p->base)) return CGCN_ERR_UNSUPPORTED;
  p->nwords = (int)((n_window_bins + 31) / 32) + 1;   // one zero word behind the last bit
  p->lds = p->nwords <= HIC_UP_LDS_WORDS;
  p->wtiles = tiles_of(M, HIC_UP_WTILE);
  WsBump w = {p->base.total - 256};   // behind the sibling's buffers
  p->o_wcounts = w.take((size_t)p->wtiles * 4);
  p->o_woff = w.take((size_t)p->wtiles * 8);
  p->tab_bytes = ws_align((size_t)p->nwords * 8) + 256;   // bitmap, rank table, the off-grid flag
  p->o_tab = w.take(p->tab_bytes);
  p->total = w.o + 256;
  return CGCN_OK;
}

// the tables of one call, and the grid of its persistent filter passes
static int hic_up_tables(hipStream_t st, const HicUpPlan& p, char* w, const int32_t* window_start, int N, int window_bp,
                         long long n_window_bins, unsigned* grid) {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return CGCN_ERR_LAUNCH;
  const long long wgs = (p.wtiles + HIC_UP_WAVES - 1) / HIC_UP_WAVES, cap = 2ll * (cus < 1 ? 1 : cus);
  *grid = (unsigned)(wgs < cap ? wgs : cap);
  unsigned* tab = (unsigned*)(w + p.o_tab);
  if (hipMemsetAsync(tab, 0, p.tab_bytes, st) != hipSuccess) return CGCN_ERR_LAUNCH;
  if (N > 0)
    hipLaunchKernelGGL(k_hic_up_bits, dim3((unsigned)tiles_of(N, 256)), dim3(256), 0, st, window_start, N, window_bp, n_window_bins,
                       tab, (int*)(w + p.o_tab + p.tab_bytes - 256));
  hipLaunchKernelGGL(k_hic_up_rank, dim3(1), dim3(1024), 0, st, p.nwords, (const unsigned*)tab, (int*)(tab + p.nwords));
  return CGCN_OK;
}

// the minimum gap and the expected vector of the distance-aware entry points; on = false: the passes as they were
struct HicDist {
  bool on;
  long long min_d;
  const double* ex;
  long long n_ex;
};

template <bool WRITE>
static void hic_up_filter(hipStream_t st, const HicUpPlan& p, unsigned grid, char* w, long long M, const int32_t* pos1,
                          const int32_t* pos2, const double* count, const double* norm, long long n_bins, int res, int wbp,
                          const int32_t* ws, int N, long long nbits, long long capacity, u64* keys, int2* ij, const HicDist& dx) {
  const unsigned* tab = (const unsigned*)(w + p.o_tab);
  const int* flag = (const int*)(w + p.o_tab + p.tab_bytes - 256);
  int* counts = (int*)(w + p.o_wcounts);
  const long long* off = (const long long*)(w + p.o_woff);
  if (dx.on) {
    if (p.lds)
      hipLaunchKernelGGL((k_hic_filter_up_dist<WRITE, true>), dim3(grid), dim3(HIC_UP_THREADS), (size_t)p.nwords * 8, st, M, pos1, pos2,
                         count, norm, n_bins, res, wbp, p.up, ws, N, tab, p.nwords, nbits, flag, p.wtiles, counts, off, capacity, keys, ij,
                         dx.min_d, dx.ex, dx.n_ex);
    else
      hipLaunchKernelGGL((k_hic_filter_up_dist<WRITE, false>), dim3(grid), dim3(HIC_UP_THREADS), 0, st, M, pos1, pos2, count, norm,
                         n_bins, res, wbp, p.up, ws, N, tab, p.nwords, nbits, flag, p.wtiles, counts, off, capacity, keys, ij, dx.min_d,
                         dx.ex, dx.n_ex);
    return;
  }
  if (p.lds)
    hipLaunchKernelGGL((k_hic_filter_up<WRITE, true>), dim3(grid), dim3(HIC_UP_THREADS), (size_t)p.nwords * 8, st, M, pos1, pos2, count,
                       norm, n_bins, res, wbp, p.up, ws, N, tab, p.nwords, nbits, flag, p.wtiles, counts, off, capacity, keys, ij);
  else
    hipLaunchKernelGGL((k_hic_filter_up<WRITE, false>), dim3(grid), dim3(HIC_UP_THREADS), 0, st, M, pos1, pos2, count, norm, n_bins,
                       res, wbp, p.up, ws, N, tab, p.nwords, nbits, flag, p.wtiles, counts, off, capacity, keys, ij);
}

extern "C" size_t cgcn_hic_workspace_bytes(long long M, int N, long long capacity, long long K) {
  HicPlan p;
  return hic_plan(M, N, capacity, K, &p) ? p.total : 0;
}

static int hic_count_impl(cgcn_stream_t stream, long long M, const int32_t* pos1, const int32_t* pos2, const int32_t* window_start,
                          int N, void* workspace, size_t workspace_bytes, long long* n_survivors, const HicDist& dx) {
  if (M < 0 || N < 0 || !n_survivors || dx.min_d < 0) return CGCN_ERR_BAD_ARG;
  if (M > 0 && (!pos1 || !pos2 || !workspace)) return CGCN_ERR_BAD_ARG;
  if (N > 0 && !window_start) return CGCN_ERR_BAD_ARG;
  HicPlan p;
  if (!hic_plan(M, N, 0, 0, &p)) return CGCN_ERR_UNSUPPORTED;
  if (workspace_bytes < p.total) return CGCN_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (M == 0) return hipMemsetAsync(n_survivors, 0, 8, st) == hipSuccess ? CGCN_OK : CGCN_ERR_LAUNCH;
  char* w = ws_base(workspace);
  int* counts = (int*)(w + p.o_counts);
  long long* off = (long long*)(w + p.o_off);
  if (dx.on)
    hipLaunchKernelGGL(k_hic_filter_dist<false>, dim3((unsigned)p.tilesM), dim3(HIC_THREADS), 0, st, M, pos1, pos2,
                       (const double*)nullptr, (const double*)nullptr, 0ll, 1, window_start, N, counts, (const long long*)nullptr, 0ll,
                       (u64*)nullptr, (int2*)nullptr, dx.min_d, (const double*)nullptr, 0ll);
  else
    hipLaunchKernelGGL(k_hic_filter<false>, dim3((unsigned)p.tilesM), dim3(HIC_THREADS), 0, st, M, pos1, pos2, (const double*)nullptr,
                       (const double*)nullptr, 0ll, 1, window_start, N, counts, (const long long*)nullptr, 0ll, (u64*)nullptr,
                       (int2*)nullptr);
  hipLaunchKernelGGL(k_tile_scan<>, dim3(1), dim3(1024), 0, st, (int)p.tilesM, (const int*)counts, off, n_survivors, (int*)nullptr, 0ll);
  return launch_status();
}

static int hic_build_impl(cgcn_stream_t stream, long long M, const int32_t* pos1, const int32_t* pos2, const double* count,
                          const double* norm, long long n_bins, int resolution_bp, const int32_t* window_start, int N, long long K,
                          long long capacity, void* workspace, size_t workspace_bytes, int32_t* rowptr_out, int32_t* col_out,
                          int32_t* nnz_out, long long* n_survivors, const HicDist& dx) {
  if (M < 0 || N < 0 || K < 0 || capacity < 0 || n_bins < 0 || !rowptr_out || !nnz_out || !n_survivors || !workspace)
    return CGCN_ERR_BAD_ARG;
  if (M > 0 && (!pos1 || !pos2 || !count)) return CGCN_ERR_BAD_ARG;
  if (N > 0 && !window_start) return CGCN_ERR_BAD_ARG;
  if (norm && (resolution_bp < 1 || n_bins < 1)) return CGCN_ERR_BAD_ARG;
  if (dx.min_d < 0 || dx.n_ex < 0 || (dx.ex && (resolution_bp < 1 || dx.n_ex < 1))) return CGCN_ERR_BAD_ARG;
  HicPlan p;
  if (!hic_plan(M, N, capacity, K, &p)) return CGCN_ERR_UNSUPPORTED;
  if (p.half > 0 && !col_out) return CGCN_ERR_BAD_ARG;
  if (workspace_bytes < p.total) return CGCN_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* w = ws_base(workspace);
  int* counts = (int*)(w + p.o_counts);
  long long* off = (long long*)(w + p.o_off);
  u64* keyA = (u64*)(w + p.o_keyA);
  int2* ij = (int2*)(w + p.o_ij);
  if (hipMemsetAsync(rowptr_out, 0, ((size_t)N + 1) * 4, st) != hipSuccess) return CGCN_ERR_LAUNCH;
  if (hipMemsetAsync(nnz_out, 0, 4, st) != hipSuccess) return CGCN_ERR_LAUNCH;
  if (M == 0) return hipMemsetAsync(n_survivors, 0, 8, st) == hipSuccess ? CGCN_OK : CGCN_ERR_LAUNCH;
  const int res = (norm || dx.ex) ? resolution_bp : 1;
  if (dx.on)
    hipLaunchKernelGGL(k_hic_filter_dist<false>, dim3((unsigned)p.tilesM), dim3(HIC_THREADS), 0, st, M, pos1, pos2, count, norm, n_bins,
                       res, window_start, N, counts, (const long long*)nullptr, 0ll, (u64*)nullptr, (int2*)nullptr, dx.min_d, dx.ex,
                       dx.n_ex);
  else
    hipLaunchKernelGGL(k_hic_filter<false>, dim3((unsigned)p.tilesM), dim3(HIC_THREADS), 0, st, M, pos1, pos2, count, norm, n_bins, res,
                       window_start, N, counts, (const long long*)nullptr, 0ll, (u64*)nullptr, (int2*)nullptr);
  hipLaunchKernelGGL(k_tile_scan<>, dim3(1), dim3(1024), 0, st, (int)p.tilesM, (const int*)counts, off, n_survivors, (int*)nullptr, 0ll);
  if (p.half == 0) return launch_status();   // no room for a record (capacity or K is 0): the empty graph
  if (dx.on)
    hipLaunchKernelGGL(k_hic_filter_dist<true>, dim3((unsigned)p.tilesM), dim3(HIC_THREADS), 0, st, M, pos1, pos2, count, norm, n_bins,
                       res, window_start, N, (int*)nullptr, (const long long*)off, capacity, keyA, ij, dx.min_d, dx.ex, dx.n_ex);
  else
    hipLaunchKernelGGL(k_hic_filter<true>, dim3((unsigned)p.tilesM), dim3(HIC_THREADS), 0, st, M, pos1, pos2, count, norm, n_bins, res,
                       window_start, N, (int*)nullptr, (const long long*)off, capacity, keyA, ij);
  return hic_select_and_csr(st, p, w, N, K, capacity, rowptr_out, col_out, nnz_out, n_survivors);
}

extern "C" size_t cgcn_hic_up_workspace_bytes(long long M, int N, long long capacity, long long K, int resolution_bp, int window_bp,
                                   long long n_window_bins) {
  HicUpPlan p;
  return hic_up_plan(M, N, capacity, K, resolution_bp, window_bp, n_window_bins, &p) == CGCN_OK ? p.total : 0;
}

static int hic_count_up_impl(cgcn_stream_t stream, long long M, const int32_t* pos1, const int32_t* pos2,
                             const int32_t* window_start, int N, int resolution_bp, int window_bp, long long n_window_bins,
                             void* workspace, size_t workspace_bytes, long long* n_survivors, const HicDist& dx) {
  if (M < 0 || N < 0 || !n_survivors || dx.min_d < 0) return CGCN_ERR_BAD_ARG;
  if (M > 0 && (!pos1 || !pos2 || !workspace)) return CGCN_ERR_BAD_ARG;
  if (N > 0 && !window_start) return CGCN_ERR_BAD_ARG;
  HicUpPlan p;
  const int rc = hic_up_plan(M, N, 0, 0, resolution_bp, window_bp, n_window_bins, &p);
  if (rc != CGCN_OK) return rc;
  if (workspace_bytes < p.total) return CGCN_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (M == 0) return hipMemsetAsync(n_survivors, 0, 8, st) == hipSuccess ? CGCN_OK : CGCN_ERR_LAUNCH;
  char* w = ws_base(workspace);
  unsigned grid = 1;
  if (hic_up_tables(st, p, w, window_start, N, window_bp, n_window_bins, &grid) != CGCN_OK) return CGCN_ERR_LAUNCH;
  hic_up_filter<false>(st, p, grid, w, M, pos1, pos2, nullptr, nullptr, 0ll, resolution_bp, window_bp, window_start, N, n_window_bins,
                       0ll, nullptr, nullptr, dx);
  hipLaunchKernelGGL(k_tile_scan<>, dim3(1), dim3(1024), 0, st, (int)p.wtiles, (const int*)(w + p.o_wcounts), (long long*)(w + p.o_woff),
                     n_survivors, (int*)nullptr, 0ll);
  return launch_status();
}

static int hic_build_up_impl(cgcn_stream_t stream, long long M, const int32_t* pos1, const int32_t* pos2, const double* count,
                             const double* norm, long long n_bins, int resolution_bp, int window_bp, long long n_window_bins,
                             const int32_t* window_start, int N, long long K, long long capacity, void* workspace,
                             size_t workspace_bytes, int32_t* rowptr_out, int32_t* col_out, int32_t* nnz_out, long long* n_survivors,
                             const HicDist& dx) {
  if (M < 0 || N < 0 || K < 0 || capacity < 0 || n_bins < 0 || !rowptr_out || !nnz_out || !n_survivors || !workspace)
    return CGCN_ERR_BAD_ARG;
  if (M > 0 && (!pos1 || !pos2 || !count)) return CGCN_ERR_BAD_ARG;
  if (N > 0 && !window_start) return CGCN_ERR_BAD_ARG;
  if (norm && n_bins < 1) return CGCN_ERR_BAD_ARG;
  if (dx.min_d < 0 || dx.n_ex < 0 || (dx.ex && dx.n_ex < 1)) return CGCN_ERR_BAD_ARG;
  HicUpPlan u;
  const int rc = hic_up_plan(M, N, capacity, K, resolution_bp, window_bp, n_window_bins, &u);
  if (rc != CGCN_OK) return rc;
  const HicPlan& p = u.base;
  if (p.half > 0 && !col_out) return CGCN_ERR_BAD_ARG;
  if (workspace_bytes < u.total) return CGCN_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* w = ws_base(workspace);
  u64* keyA = (u64*)(w + p.o_keyA);
  int2* ij = (int2*)(w + p.o_ij);
  if (hipMemsetAsync(rowptr_out, 0, ((size_t)N + 1) * 4, st) != hipSuccess) return CGCN_ERR_LAUNCH;
  if (hipMemsetAsync(nnz_out, 0, 4, st) != hipSuccess) return CGCN_ERR_LAUNCH;
  if (M == 0) return hipMemsetAsync(n_survivors, 0, 8, st) == hipSuccess ? CGCN_OK : CGCN_ERR_LAUNCH;
  unsigned grid = 1;
  if (hic_up_tables(st, u, w, window_start, N, window_bp, n_window_bins, &grid) != CGCN_OK) return CGCN_ERR_LAUNCH;
  hic_up_filter<false>(st, u, grid, w, M, pos1, pos2, count, norm, n_bins, resolution_bp, window_bp, window_start, N, n_window_bins,
                       0ll, nullptr, nullptr, dx);
  hipLaunchKernelGGL(k_tile_scan<>, dim3(1), dim3(1024), 0, st, (int)u.wtiles, (const int*)(w + u.o_wcounts), (long long*)(w + u.o_woff),
                     n_survivors, (int*)nullptr, 0ll);
  if (p.half == 0) return launch_status();   // no room for a record (capacity or K is 0): the empty graph
  hic_up_filter<true>(st, u, grid, w, M, pos1, pos2, count, norm, n_bins, resolution_bp, window_bp, window_start, N, n_window_bins,
                      capacity, keyA, ij, dx);
  return hic_select_and_csr(st, p, w, N, K, capacity, rowptr_out, col_out, nnz_out, n_survivors);
}


static const HicDist HIC_PLAIN = {false, 0ll, nullptr, 0ll};

extern "C" {

int cgcn_hic_count(cgcn_stream_t stream, long long M, const int32_t* pos1, const int32_t* pos2, const int32_t* window_start,
                   int N, void* workspace, size_t workspace_bytes, long long* n_survivors) {
  return hic_count_impl(stream, M, pos1, pos2, window_start, N, workspace, workspace_bytes, n_survivors, HIC_PLAIN);
}

int cgcn_hic_build(cgcn_stream_t stream, long long M, const int32_t* pos1, const int32_t* pos2, const double* count,
                   const double* norm, long long n_bins, int resolution_bp, const int32_t* window_start, int N, long long K,
                   long long capacity, void* workspace, size_t workspace_bytes, int32_t* rowptr_out, int32_t* col_out,
                   int32_t* nnz_out, long long* n_survivors) {
  return hic_build_impl(stream, M, pos1, pos2, count, norm, n_bins, resolution_bp, window_start, N, K, capacity, workspace,
                        workspace_bytes, rowptr_out, col_out, nnz_out, n_survivors, HIC_PLAIN);
}

int cgcn_hic_count_up(cgcn_stream_t stream, long long M, const int32_t* pos1, const int32_t* pos2, const int32_t* window_start,
                      int N, int resolution_bp, int window_bp, long long n_window_bins, void* workspace, size_t workspace_bytes,
                      long long* n_survivors) {
  return hic_count_up_impl(stream, M, pos1, pos2, window_start, N, resolution_bp, window_bp, n_window_bins, workspace,
                           workspace_bytes, n_survivors, HIC_PLAIN);
}

int cgcn_hic_build_up(cgcn_stream_t stream, long long M, const int32_t* pos1, const int32_t* pos2, const double* count,
                      const double* norm, long long n_bins, int resolution_bp, int window_bp, long long n_window_bins,
                      const int32_t* window_start, int N, long long K, long long capacity, void* workspace, size_t workspace_bytes,
                      int32_t* rowptr_out, int32_t* col_out, int32_t* nnz_out, long long* n_survivors) {
  return hic_build_up_impl(stream, M, pos1, pos2, count, norm, n_bins, resolution_bp, window_bp, n_window_bins, window_start, N, K,
                           capacity, workspace, workspace_bytes, rowptr_out, col_out, nnz_out, n_survivors, HIC_PLAIN);
}

// The distance-aware forms: the same passes with the minimum gap min_distance_bp >= 0 and, in the
// builds, the expected vector (NULL: none).  Workspaces and sizes as for the four functions above.
int cgcn_hic_count_dist(cgcn_stream_t stream, long long M, const int32_t* pos1, const int32_t* pos2, const int32_t* window_start,
                        int N, long long min_distance_bp, void* workspace, size_t workspace_bytes, long long* n_survivors) {
  const HicDist dx = {true, min_distance_bp, nullptr, 0ll};
  return hic_count_impl(stream, M, pos1, pos2, window_start, N, workspace, workspace_bytes, n_survivors, dx);
}

int cgcn_hic_build_dist(cgcn_stream_t stream, long long M, const int32_t* pos1, const int32_t* pos2, const double* count,
                        const double* norm, long long n_bins, int resolution_bp, const int32_t* window_start, int N, long long K,
                        long long capacity, long long min_distance_bp, const double* expected, long long n_expected,
                        void* workspace, size_t workspace_bytes, int32_t* rowptr_out, int32_t* col_out, int32_t* nnz_out,
                        long long* n_survivors) {
  const HicDist dx = {true, min_distance_bp, expected, n_expected};
  return hic_build_impl(stream, M, pos1, pos2, count, norm, n_bins, resolution_bp, window_start, N, K, capacity, workspace,
                        workspace_bytes, rowptr_out, col_out, nnz_out, n_survivors, dx);
}

int cgcn_hic_count_up_dist(cgcn_stream_t stream, long long M, const int32_t* pos1, const int32_t* pos2,
                           const int32_t* window_start, int N, int resolution_bp, int window_bp, long long n_window_bins,
                           long long min_distance_bp, void* workspace, size_t workspace_bytes, long long* n_survivors) {
  const HicDist dx = {true, min_distance_bp, nullptr, 0ll};
  return hic_count_up_impl(stream, M, pos1, pos2, window_start, N, resolution_bp, window_bp, n_window_bins, workspace,
                           workspace_bytes, n_survivors, dx);
}

int cgcn_hic_build_up_dist(cgcn_stream_t stream, long long M, const int32_t* pos1, const int32_t* pos2, const double* count,
                           const double* norm, long long n_bins, int resolution_bp, int window_bp, long long n_window_bins,
                           const int32_t* window_start, int N, long long K, long long capacity, long long min_distance_bp,
                           const double* expected, long long n_expected, void* workspace, size_t workspace_bytes,
                           int32_t* rowptr_out, int32_t* col_out, int32_t* nnz_out, long long* n_survivors) {
  const HicDist dx = {true, min_distance_bp, expected, n_expected};
  return hic_build_up_impl(stream, M, pos1, pos2, count, norm, n_bins, resolution_bp, window_bp, n_window_bins, window_start, N, K,
                           capacity, workspace, workspace_bytes, rowptr_out, col_out, nnz_out, n_survivors, dx);
}

}  // extern "C"
