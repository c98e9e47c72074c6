// chromegcn_amd/csrc/cgcn_nullgraph.hip -- distance- and degree-matched random contact graphs.
//
// The rule is the docstring of chromegcn_amd/nullgraph.py; null_graph_host restates it in numpy and every output of this
// unit is held to that restatement bit for bit (tests/test_gpu_nullgraph.py).  Integer arithmetic only.
//
// Nothing here knows a data-dependent size on the host: the edge count m, the token count T and the number of output
// entries live in a block of device counters, every array is sized by what the host does know (nnz of the input, the
// caller's capacity) and every grid covers that bound.  Order is restored by sorting, so every pass that appends does it
// with an integer atomic cursor and no pass depends on the order workgroups run in:
//   k_ng_edges       a wave per row: upper entries counted (m), the distance histogram c_d by integer atomics; 'degree'
//                    keeps the per-row counts, k_tile_scan turns them into edge indices and k_ng_stubs (same walk, ballot
//                    ranks) numbers the stubs in storage order
//   k_ng_classes     'distance': k_d and the flag extent n_d of complemented classes; two k_tile_scan give the token bases
//                    and the flag-segment bases
//   k_ng_init        the tokens' classes (binary search in the bases) and their first keys
//   per round        rocprim::radix_sort_keys of (class, position, token) -- keys alone, the token index is the low end, so
//                    the first key of a run of equal (class, position) is the winner -- then k_ng_round: every other key of
//                    a run is a loser, increments its attempt and rewrites its own key in the UNSORTED array (the sort reads
//                    it again next round; one thread per token, no race).  The last round counts the losers as unplaced and
//                    emits the winners: an edge, or a flag in the segment of a complemented class.  The sorts of a round
//                    without losers still run (their size is a host fact); its k_ng_round changes nothing.
//   k_ng_free        complemented classes: every flag-less position of a segment is an edge
//   'degree'         one sort of (hash, stub), k_ng_pairs (loops out), one sort of the pairs, k_ng_unique (repeats out)
//   final            both directions were appended as (row, col) keys: one sort, then k_ng_write cuts the columns and finds
//                    every rowptr by binary search
// All stores are ordinary vector stores; every index read from an array is checked against its table before it forms an
// address.
#include <cstring>  // rocprim 4.x headers use memset without including it
#include <rocprim/rocprim.hpp>

#include "cgcn_compact.hpp"

#define NG_THREADS 256
enum { NG_M = 0, NG_T, NG_UNPLACED, NG_COMP, NG_LOOPS, NG_REPEATS, NG_ROUNDS, NG_FLAGS, NG_OUT, NG_FEXT, NG_WORDS = 16 };
enum { NG_FLAG_OVERRUN = 1, NG_FLAG_UNSUPPORTED = 2, NG_FLAG_BAD_INDEX = 4 };
#define NG_PAD (~0ull)

struct NgBits {
  int bN, bT;   // bits of a window index; of a token (or stub) index
};

// key(seed, attempt, stream) of the rule: dropout_key with the step counter replaced by the attempt (its high half is 0)
__device__ __forceinline__ uint32_t ng_key(u64 seed, uint32_t attempt, uint32_t stream) {
  uint32_t k = mix32((uint32_t)seed ^ 0x9E3779B9u);
  k = mix32(k ^ (uint32_t)(seed >> 32));
  k = mix32(k + attempt * 0x85EBCA6Bu);
  return mix32(k ^ (stream * 0xC2B2AE35u));
}
__device__ __forceinline__ uint32_t ng_draw(uint32_t t, uint32_t key, uint32_t R) {
  return (uint32_t)(((u64)mix32(t * 0x9E3779B1u + key) * (u64)R) >> 32);
}

// the (class, position) code of token t at `attempt`: distance (d, p), uniform (min, max); false when the token has none
template <int MODEL>
__device__ __forceinline__ bool ng_code(int n, u64 seed, int t, int attempt, int d, int bN, u64& code) {
  if (MODEL == CGCN_NULL_DISTANCE) {
    if (d < 1 || d >= n) return false;
    const uint32_t p = ng_draw((uint32_t)t, ng_key(seed, (uint32_t)attempt, 1u), (uint32_t)(n - d));
    code = ((u64)d << bN) | p;
  } else {
    if (n < 2) return false;
    const uint32_t u = ng_draw((uint32_t)t, ng_key(seed, (uint32_t)attempt, 3u), (uint32_t)n);
    uint32_t w = ng_draw((uint32_t)t, ng_key(seed, (uint32_t)attempt, 4u), (uint32_t)(n - 1));
    if (w >= u) ++w;
    code = ((u64)min(u, w) << bN) | max(u, w);
  }
  return true;
}

// the last d in [0, n) with base[d] <= x (base ascending, base[0] = 0 <= x)
__device__ __forceinline__ int ng_last_le(const long long* __restrict__ base, int n, long long x) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if (base[mid] <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// both directions of the edge (lo, hi) as (row, col) keys behind the cursor
__device__ __forceinline__ void ng_append(u64* __restrict__ out, long long capacity, int* ctr, int lo, int hi, int bN) {
  const long long at = (long long)atomicAdd(&ctr[NG_OUT], 2);
  if (at < 0 || at + 2 > capacity) {
    atomicOr(&ctr[NG_FLAGS], NG_FLAG_OVERRUN);
    return;
  }
  out[at] = ((u64)lo << bN) | (u64)hi;
  out[at + 1] = ((u64)hi << bN) | (u64)lo;
}

// ---------------------------------------------------------------------------------------------------------------------
// A wave per row over the stored entries.  STUBS = false: count the upper entries (ctr[NG_M], row_count) and, for
// 'distance', add them to the histogram.  STUBS = true ('degree', behind the scan of row_count): edge e = ebase[i] + rank in
// storage order owns the stubs 2e (window i) and 2e + 1 (window j); their nodes and sort keys are written.
template <bool STUBS>
__global__ __launch_bounds__(NG_THREADS) void k_ng_edges(int n, long long nnz, const int* __restrict__ rowptr,
                                                         const int* __restrict__ col, int model, int* __restrict__ hist,
                                                         int* __restrict__ row_count, const long long* __restrict__ ebase,
                                                         long long cap, int* __restrict__ node, u64* __restrict__ keys, u64 seed,
                                                         int bT, int* __restrict__ ctr) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int i = blockIdx.x * (NG_THREADS / WAVE) + threadIdx.x / WAVE;
  if (i >= n) return;
  long long b = rowptr[i], e = rowptr[i + 1];
  b = b < 0 ? 0 : (b > nnz ? nnz : b);
  e = e < b ? b : (e > nnz ? nnz : e);
  const uint32_t hkey = STUBS ? ng_key(seed, 0u, 2u) : 0u;
  long long run = STUBS ? ebase[i] : 0;
  int bad = 0;
  for (long long p0 = b; p0 < e; p0 += WAVE) {
    const long long p = p0 + lane;
    int j = -1;
    if (p < e) {
      j = col[p];
      if (j < 0 || j >= n) {
        bad = 1;
        j = -1;
      }
    }
    const bool upper = j > i;
    const u64 m = __ballot(upper);
    if (upper) {
      if (!STUBS) {
        if (model == CGCN_NULL_DISTANCE) atomicAdd(&hist[j - i], 1);
      } else {
        const long long ed = run + __popcll(m & ((1ull << lane) - 1ull));
        if (ed >= 0 && ed < cap) {
          const uint32_t s = (uint32_t)(2 * ed);
          node[s] = i;
          node[s + 1] = j;
          keys[s] = ((u64)mix32(s * 0x9E3779B1u + hkey) << bT) | s;
          keys[s + 1] = ((u64)mix32((s + 1u) * 0x9E3779B1u + hkey) << bT) | (s + 1u);
        }
      }
    }
    run += __popcll(m);
  }
  if (!STUBS) {
    if (lane == 0) {
      if (row_count) row_count[i] = (int)run;
      if (run) atomicAdd(&ctr[NG_M], (int)run);
    }
    if (bad) atomicOr(&ctr[NG_FLAGS], NG_FLAG_BAD_INDEX);
  }
}

// 'distance': tokens and flag extent of every class
__global__ __launch_bounds__(NG_THREADS) void k_ng_classes(int n, const int* __restrict__ hist, int* __restrict__ kd,
                                                           int* __restrict__ fext, int* __restrict__ ctr) {
  const int d = blockIdx.x * NG_THREADS + threadIdx.x;
  if (d >= n) return;
  int k = 0, f = 0;
  if (d >= 1) {
    const int nd = n - d;
    const int c = min(max(hist[d], 0), nd);   // (more than n_d only for an input with repeated entries)
    if (2ll * c > nd) {
      k = nd - c;
      f = nd;
      atomicAdd(&ctr[NG_COMP], 1);
    } else {
      k = c;
    }
  }
  kd[d] = k;
  fext[d] = f;
}

// the token count of the model (behind the scans): distance ctr[NG_T] as scanned, uniform m -- or 0 with the unsupported flag
template <int MODEL>
__device__ __forceinline__ int ng_tokens(int n, const int* __restrict__ ctr, long long cap, bool& unsupported) {
  unsupported = false;
  long long T;
  if (MODEL == CGCN_NULL_DISTANCE) {
    T = ctr[NG_T];
  } else {
    T = ctr[NG_M];
    if (T > 0 && (n < 2 || 4ll * T > (long long)n * (n - 1))) {
      unsupported = true;
      T = 0;
    }
  }
  return (int)(T < 0 ? 0 : (T > cap ? cap : T));
}

template <int MODEL>
__global__ __launch_bounds__(NG_THREADS) void k_ng_init(int n, long long cap, const long long* __restrict__ tbase, u64 seed,
                                                        NgBits B, int* __restrict__ cls, int* __restrict__ att,
                                                        u64* __restrict__ keys, int* __restrict__ ctr) {
  const long long t = (long long)blockIdx.x * NG_THREADS + threadIdx.x;
  if (t >= cap) return;
  bool unsupported;
  const int T = ng_tokens<MODEL>(n, ctr, cap, unsupported);
  if (t == 0) {
    if (unsupported) atomicOr(&ctr[NG_FLAGS], NG_FLAG_UNSUPPORTED);
    if (MODEL == CGCN_NULL_UNIFORM) ctr[NG_T] = T;
  }
  u64 k = NG_PAD, code;
  if (t < T) {
    const int d = MODEL == CGCN_NULL_DISTANCE ? ng_last_le(tbase, n, t) : 0;
    if (MODEL == CGCN_NULL_DISTANCE) cls[t] = d;
    att[t] = 0;
    if (ng_code<MODEL>(n, seed, (int)t, 0, d, B.bN, code)) k = (code << B.bT) | (u64)t;
  }
  keys[t] = k;
}

// One round over the SORTED keys.  A key whose (class, position) equals its predecessor's is a loser.  Before the last
// round it redraws; in the last round it is unplaced and the winners are emitted.
template <int MODEL>
__global__ __launch_bounds__(NG_THREADS) void k_ng_round(int n, long long cap, const u64* __restrict__ sorted, u64* __restrict__ keys,
                                                         int* __restrict__ att, const int* __restrict__ cls, u64 seed, NgBits B,
                                                         int round, int last, const int* __restrict__ fext,
                                                         const long long* __restrict__ fbase, unsigned char* __restrict__ flags,
                                                         long long flag_cap, u64* __restrict__ out, long long capacity,
                                                         int* __restrict__ ctr) {
  const long long i = (long long)blockIdx.x * NG_THREADS + threadIdx.x;
  if (i >= cap) return;
  const u64 k = sorted[i];
  if (k == NG_PAD) return;
  const int T = min(max(ctr[NG_T], 0), (int)cap);
  const int t = (int)(k & ((1ull << B.bT) - 1ull));
  if (t >= T) return;
  const u64 code = k >> B.bT;
  const bool loser = i > 0 && (sorted[i - 1] >> B.bT) == code;
  if (loser) {
    atomicMax(&ctr[NG_ROUNDS], round + 1);
    if (last) {
      atomicAdd(&ctr[NG_UNPLACED], 1);
    } else {
      const int a = att[t] + 1;
      att[t] = a;
      u64 c2;
      const int d = MODEL == CGCN_NULL_DISTANCE ? cls[t] : 0;
      keys[t] = ng_code<MODEL>(n, seed, t, a, d, B.bN, c2) ? (c2 << B.bT) | (u64)t : NG_PAD;
    }
    return;
  }
  if (!last) return;
  const int hi_part = (int)(code >> B.bN), lo_part = (int)(code & ((1ull << B.bN) - 1ull));
  if (MODEL == CGCN_NULL_DISTANCE) {
    const int d = hi_part, p = lo_part;
    if (d < 1 || d >= n || p >= n - d) return;
    if (fext[d] > 0) {
      const long long at = fbase[d] + p;
      if (at >= 0 && at < flag_cap) flags[at] = 1;
    } else {
      ng_append(out, capacity, ctr, p, p + d, B.bN);
    }
  } else {
    if (hi_part < lo_part && lo_part < n) ng_append(out, capacity, ctr, hi_part, lo_part, B.bN);
  }
}

// complemented classes: every position of a flag segment without a placed hole is an edge
__global__ __launch_bounds__(NG_THREADS) void k_ng_free(int n, long long flag_cap, const int* __restrict__ fext,
                                                        const long long* __restrict__ fbase, const unsigned char* __restrict__ flags,
                                                        int bN, u64* __restrict__ out, long long capacity, int* __restrict__ ctr) {
  const long long x = (long long)blockIdx.x * NG_THREADS + threadIdx.x;
  const long long ext = min((long long)max(ctr[NG_FEXT], 0), flag_cap);
  if (x >= ext || flags[x]) return;
  const int d = ng_last_le(fbase, n, x);
  const long long p = x - fbase[d];
  if (d < 1 || p < 0 || p >= fext[d] || p >= n - d) return;
  ng_append(out, capacity, ctr, (int)p, (int)p + d, bN);
}

// 'degree': the sorted stubs 2q and 2q + 1 form pair q
__global__ __launch_bounds__(NG_THREADS) void k_ng_pairs(int n, long long cap, const u64* __restrict__ sorted,
                                                         const int* __restrict__ node, NgBits B, u64* __restrict__ pairs,
                                                         int* __restrict__ ctr) {
  const long long q = (long long)blockIdx.x * NG_THREADS + threadIdx.x;
  if (q >= cap) return;
  const long long m = min((long long)max(ctr[NG_M], 0), cap);
  if (q == 0) ctr[NG_T] = (int)(2 * m);
  u64 k = NG_PAD;
  if (q < m) {
    const u64 mask = (1ull << B.bT) - 1ull;
    const u64 k1 = sorted[2 * q], k2 = sorted[2 * q + 1];
    const long long s1 = (long long)(k1 & mask), s2 = (long long)(k2 & mask);
    if (k1 != NG_PAD && k2 != NG_PAD && s1 < 2 * m && s2 < 2 * m) {
      const int u = node[s1], v = node[s2];
      if (u == v) {
        atomicAdd(&ctr[NG_LOOPS], 1);
      } else if (u >= 0 && u < n && v >= 0 && v < n) {
        k = ((u64)min(u, v) << B.bN) | (u64)max(u, v);
      }
    }
  }
  pairs[q] = k;
}

__global__ __launch_bounds__(NG_THREADS) void k_ng_unique(int n, long long cap, const u64* __restrict__ sorted, int bN,
                                                          u64* __restrict__ out, long long capacity, int* __restrict__ ctr) {
  const long long q = (long long)blockIdx.x * NG_THREADS + threadIdx.x;
  if (q >= cap) return;
  const u64 k = sorted[q];
  if (k == NG_PAD) return;
  if (q > 0 && sorted[q - 1] == k) {
    atomicAdd(&ctr[NG_REPEATS], 1);
    return;
  }
  const int lo = (int)(k >> bN), hi = (int)(k & ((1ull << bN) - 1ull));
  if (lo < hi && hi < n) ng_append(out, capacity, ctr, lo, hi, bN);
}

// the sorted (row, col) keys -> col, rowptr (binary search per row) and the counters
__global__ __launch_bounds__(NG_THREADS) void k_ng_write(int n, long long capacity, const u64* __restrict__ sorted, int bN,
                                                         const int* __restrict__ ctr, int* __restrict__ rowptr,
                                                         int* __restrict__ col, long long* __restrict__ sizes) {
  const long long i = (long long)blockIdx.x * NG_THREADS + threadIdx.x;
  const long long E = min((long long)max(ctr[NG_OUT], 0), capacity);
  if (i < capacity) col[i] = i < E ? (int)(sorted[i] & ((1ull << bN) - 1ull)) : 0;
  if (i <= n) {
    const u64 want = (u64)i << bN;   // the first key of row i or behind
    long long lo = 0, hi = E;
    while (lo < hi) {
      const long long mid = lo + (hi - lo) / 2;
      if (sorted[mid] < want) lo = mid + 1; else hi = mid;
    }
    rowptr[i] = (int)lo;
  }
  if (i == 0) {
    sizes[0] = E;
    sizes[1] = ctr[NG_M];
    sizes[2] = E / 2;
    sizes[3] = ctr[NG_T];
    sizes[4] = ctr[NG_UNPLACED];
    sizes[5] = ctr[NG_COMP];
    sizes[6] = ctr[NG_LOOPS];
    sizes[7] = ctr[NG_REPEATS];
    sizes[8] = ctr[NG_ROUNDS];
    sizes[9] = ctr[NG_FLAGS];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
struct NgPlan {
  long long cap, nkeys, flag_cap;   // edge bound (>= 1); keys of the token / stub sorts; bytes of the flag segments
  NgBits B;
  unsigned tok_bits, out_bits;      // sorted bits of the token (stub) keys and of the (row, col) keys
  size_t temp, o_ctr, o_hist, o_kd, o_fext, o_tbase, o_fbase, o_cls, o_att, o_node, o_keyA, o_keyB, o_flags, o_outA, o_outB,
      o_temp, total;
};

static bool ng_plan(int n, long long nnz, long long capacity, int model, NgPlan* p) {
  if (n < 0 || nnz < 0 || capacity < 1) return false;
  if (model != CGCN_NULL_DISTANCE && model != CGCN_NULL_DEGREE && model != CGCN_NULL_UNIFORM) return false;
  if (n >= 2147483646 || nnz >= (1ll << 30) || capacity >= (1ll << 31)) return false;
  p->cap = nnz < 1 ? 1 : nnz;
  const bool degree = model == CGCN_NULL_DEGREE;
  p->nkeys = degree ? 2 * p->cap : p->cap;
  p->flag_cap = model == CGCN_NULL_DISTANCE ? 2 * p->cap : 0;   // complemented classes have n_d < 2 c_d: extent < 2 m
  p->B.bN = bits_for(n);
  p->B.bT = bits_for(p->nkeys);
  const int tb = degree ? 32 + p->B.bT + 1 : 2 * p->B.bN + p->B.bT + 1;   // + 1: the padding sorts behind every key
  if (tb > 64 || 2 * p->B.bN + 1 > 64) return false;
  p->tok_bits = (unsigned)tb;
  p->out_bits = (unsigned)(2 * p->B.bN + 1);
  size_t t1 = 0, t2 = 0, t3 = 0;
  (void)rocprim::radix_sort_keys(nullptr, t1, (const u64*)nullptr, (u64*)nullptr, (size_t)p->nkeys, 0u, p->tok_bits);
  (void)rocprim::radix_sort_keys(nullptr, t2, (const u64*)nullptr, (u64*)nullptr, (size_t)capacity, 0u, p->out_bits);
  if (degree) (void)rocprim::radix_sort_keys(nullptr, t3, (const u64*)nullptr, (u64*)nullptr, (size_t)p->cap, 0u, p->out_bits);
  p->temp = t1 > t2 ? t1 : t2;
  if (t3 > p->temp) p->temp = t3;
  const size_t n1 = (size_t)(n < 1 ? 1 : n);
  WsBump b = {0};
  p->o_ctr = b.take(NG_WORDS * 4);
  p->o_hist = b.take(n1 * 4);    // distance: c_d; degree: the rows' upper counts
  p->o_kd = b.take(n1 * 4);
  p->o_fext = b.take(n1 * 4);
  p->o_tbase = b.take(n1 * 8);   // distance: token bases; degree: edge bases
  p->o_fbase = b.take(n1 * 8);
  p->o_cls = b.take((size_t)p->cap * 4);
  p->o_att = b.take((size_t)p->cap * 4);
  p->o_node = b.take(degree ? (size_t)p->nkeys * 4 : 4);
  p->o_keyA = b.take((size_t)p->nkeys * 8);
  p->o_keyB = b.take((size_t)p->nkeys * 8);
  p->o_flags = b.take(p->flag_cap ? (size_t)p->flag_cap : 4);
  p->o_outA = b.take((size_t)capacity * 8);
  p->o_outB = b.take((size_t)capacity * 8);
  p->o_temp = b.take(p->temp);
  p->total = b.o + 256;
  return true;
}

static inline unsigned ng_grid(long long items) { return (unsigned)tiles_of(items, NG_THREADS); }

template <int MODEL>
static int ng_place(hipStream_t st, int n, const NgPlan& p, char* w, u64 seed, int rounds, long long capacity) {
  int* ctr = (int*)(w + p.o_ctr);
  int* cls = (int*)(w + p.o_cls);
  int* att = (int*)(w + p.o_att);
  u64* keyA = (u64*)(w + p.o_keyA);
  u64* keyB = (u64*)(w + p.o_keyB);
  const long long* tbase = (const long long*)(w + p.o_tbase);
  hipLaunchKernelGGL(k_ng_init<MODEL>, dim3(ng_grid(p.cap)), dim3(NG_THREADS), 0, st, n, p.cap, tbase, seed, p.B, cls, att, keyA, ctr);
  for (int r = 0; r < rounds; ++r) {
    size_t temp = p.temp;
    if (rocprim::radix_sort_keys((void*)(w + p.o_temp), temp, (const u64*)keyA, keyB, (size_t)p.cap, 0u, p.tok_bits, st) != hipSuccess)
      return CGCN_ERR_LAUNCH;
    hipLaunchKernelGGL(k_ng_round<MODEL>, dim3(ng_grid(p.cap)), dim3(NG_THREADS), 0, st, n, p.cap, (const u64*)keyB, keyA, att,
                       (const int*)cls, seed, p.B, r, r + 1 == rounds ? 1 : 0, (const int*)(w + p.o_fext),
                       (const long long*)(w + p.o_fbase), (unsigned char*)(w + p.o_flags), p.flag_cap, (u64*)(w + p.o_outA), capacity,
                       ctr);
  }
  return CGCN_OK;
}

extern "C" {

size_t cgcn_null_graph_workspace_bytes(int n, long long nnz, long long capacity, int model) {
  NgPlan p;
  return ng_plan(n, nnz, capacity, model, &p) ? p.total : 0;
}

int cgcn_null_graph(cgcn_stream_t stream, int n, long long nnz, const int32_t* rowptr, const int32_t* col, int model, long long seed,
                    int rounds, long long capacity, int32_t* rowptr_out, int32_t* col_out, long long* sizes, void* workspace,
                    size_t workspace_bytes) {
  if (n < 0 || nnz < 0 || capacity < 1 || rounds < 1 || !rowptr || !rowptr_out || !col_out || !sizes || !workspace)
    return CGCN_ERR_BAD_ARG;
  if (nnz > 0 && !col) return CGCN_ERR_BAD_ARG;
  if (model != CGCN_NULL_DISTANCE && model != CGCN_NULL_DEGREE && model != CGCN_NULL_UNIFORM) return CGCN_ERR_BAD_ARG;
  NgPlan p;
  if (!ng_plan(n, nnz, capacity, model, &p)) return CGCN_ERR_UNSUPPORTED;
  if (workspace_bytes < p.total) return CGCN_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* w = ws_base(workspace);
  int* ctr = (int*)(w + p.o_ctr);
  int* hist = (int*)(w + p.o_hist);
  u64* keyA = (u64*)(w + p.o_keyA);
  u64* keyB = (u64*)(w + p.o_keyB);
  u64* outA = (u64*)(w + p.o_outA);
  u64* outB = (u64*)(w + p.o_outB);
  const u64 sd = (u64)seed;
  const size_t n1 = (size_t)(n < 1 ? 1 : n);
  if (hipMemsetAsync(ctr, 0, NG_WORDS * 4, st) != hipSuccess) return CGCN_ERR_LAUNCH;
  if (hipMemsetAsync(outA, 0xFF, (size_t)capacity * 8, st) != hipSuccess) return CGCN_ERR_LAUNCH;
  if (n > 0 && nnz > 0) {
    if (hipMemsetAsync(hist, 0, n1 * 4, st) != hipSuccess) return CGCN_ERR_LAUNCH;
    const unsigned row_grid = (unsigned)tiles_of(n, NG_THREADS / WAVE);
    hipLaunchKernelGGL(k_ng_edges<false>, dim3(row_grid), dim3(NG_THREADS), 0, st, n, nnz, rowptr, col, model, hist,
                       model == CGCN_NULL_DEGREE ? hist : (int*)nullptr, (const long long*)nullptr, p.cap, (int*)nullptr, (u64*)nullptr,
                       sd, p.B.bT, ctr);
    if (model == CGCN_NULL_DEGREE) {
      long long* ebase = (long long*)(w + p.o_tbase);
      int* node = (int*)(w + p.o_node);
      if (hipMemsetAsync(keyA, 0xFF, (size_t)p.nkeys * 8, st) != hipSuccess) return CGCN_ERR_LAUNCH;
      hipLaunchKernelGGL(k_tile_scan<>, dim3(1), dim3(1024), 0, st, n, (const int*)hist, ebase, (long long*)nullptr, (int*)nullptr, 0ll);
      hipLaunchKernelGGL(k_ng_edges<true>, dim3(row_grid), dim3(NG_THREADS), 0, st, n, nnz, rowptr, col, model, (int*)nullptr,
                         (int*)nullptr, (const long long*)ebase, p.cap, node, keyA, sd, p.B.bT, ctr);
      size_t temp = p.temp;
      if (rocprim::radix_sort_keys((void*)(w + p.o_temp), temp, (const u64*)keyA, keyB, (size_t)p.nkeys, 0u, p.tok_bits, st) != hipSuccess)
        return CGCN_ERR_LAUNCH;
      u64* pairA = keyA;            // the unsorted stub keys are done with: the pair keys and their sorted copy take their place
      u64* pairB = keyA + p.cap;
      hipLaunchKernelGGL(k_ng_pairs, dim3(ng_grid(p.cap)), dim3(NG_THREADS), 0, st, n, p.cap, (const u64*)keyB, (const int*)node, p.B,
                         pairA, ctr);
      temp = p.temp;
      if (rocprim::radix_sort_keys((void*)(w + p.o_temp), temp, (const u64*)pairA, pairB, (size_t)p.cap, 0u, p.out_bits, st) != hipSuccess)
        return CGCN_ERR_LAUNCH;
      hipLaunchKernelGGL(k_ng_unique, dim3(ng_grid(p.cap)), dim3(NG_THREADS), 0, st, n, p.cap, (const u64*)pairB, p.B.bN, outA, capacity,
                         ctr);
    } else if (model == CGCN_NULL_DISTANCE) {
      int* kd = (int*)(w + p.o_kd);
      int* fext = (int*)(w + p.o_fext);
      long long* tbase = (long long*)(w + p.o_tbase);
      long long* fbase = (long long*)(w + p.o_fbase);
      if (hipMemsetAsync(w + p.o_flags, 0, (size_t)p.flag_cap, st) != hipSuccess) return CGCN_ERR_LAUNCH;
      hipLaunchKernelGGL(k_ng_classes, dim3(ng_grid(n)), dim3(NG_THREADS), 0, st, n, (const int*)hist, kd, fext, ctr);
      hipLaunchKernelGGL(k_tile_scan<>, dim3(1), dim3(1024), 0, st, n, (const int*)kd, tbase, (long long*)nullptr, ctr + NG_T, p.cap);
      hipLaunchKernelGGL(k_tile_scan<>, dim3(1), dim3(1024), 0, st, n, (const int*)fext, fbase, (long long*)nullptr, ctr + NG_FEXT,
                         p.flag_cap);
      const int rc = ng_place<CGCN_NULL_DISTANCE>(st, n, p, w, sd, rounds, capacity);
      if (rc != CGCN_OK) return rc;
      hipLaunchKernelGGL(k_ng_free, dim3(ng_grid(p.flag_cap)), dim3(NG_THREADS), 0, st, n, p.flag_cap, (const int*)fext,
                         (const long long*)fbase, (const unsigned char*)(w + p.o_flags), p.B.bN, outA, capacity, ctr);
    } else {
      const int rc = ng_place<CGCN_NULL_UNIFORM>(st, n, p, w, sd, rounds, capacity);
      if (rc != CGCN_OK) return rc;
    }
    size_t temp = p.temp;
    if (rocprim::radix_sort_keys((void*)(w + p.o_temp), temp, (const u64*)outA, outB, (size_t)capacity, 0u, p.out_bits, st) != hipSuccess)
      return CGCN_ERR_LAUNCH;
  } else {
    outB = outA;   // no edges: nothing was appended, nothing to sort
  }
  long long cover = capacity > (long long)n + 1 ? capacity : (long long)n + 1;
  hipLaunchKernelGGL(k_ng_write, dim3(ng_grid(cover)), dim3(NG_THREADS), 0, st, n, capacity, (const u64*)outB, p.B.bN, (const int*)ctr,
                     rowptr_out, col_out, sizes);
  return launch_status();
}

}  // extern "C"
