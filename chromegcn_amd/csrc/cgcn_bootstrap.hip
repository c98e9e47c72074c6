// chromegcn_amd/csrc/cgcn_bootstrap.hip -- weighted multi-label ranking sums for many weight vectors from ONE sort
// (block-bootstrap confidence intervals).
//
// The rules are the docstring of chromegcn_amd/bootstrap.py; bootstrap_weights_host and weighted_sums_host restate them in
// numpy and every output of this unit is held to them (tests/test_gpu_bootstrap.py): the weights and the integer sums bit
// for bit, the two float64 sums to their rounding.
//
//   sort      64-bit keys [label | descending order-preserving image of the score | target | window index], ONE
//             rocprim::radix_sort_keys; k_bs_order cuts every sorted key down to one word per element:
//             window index | target << 30 | run end << 31.  A run end depends on the scores only.
//   weights   the tile [G][n][64] bytes: group g = replicates 64 g .. 64 g + 63, one 64-byte row per window.  From the rule:
//             an integer-atomic histogram of the block starts (same layout, int32: exact in any order), then the circular
//             sliding sum over L_s.  Explicit int32 weights [R, n] are transposed into the same tile through LDS.
//   walk      one wave per (label, group), one replicate per lane: k_bs_walk reads a label's list (64 elements per vector
//             load, then lane by lane as scalars), issues BS_BATCH row loads of the tile ahead of the arithmetic -- the addresses
//             depend on the list only -- and every lane keeps its own tp, TOT, previous point and sums.  No scan, no cross-lane
//             traffic, no atomics; a run end is a scalar branch.
// A weight is a byte and n < 2^23, so every TOT is below 255 * 2^23 < 2^31 and A below 2^62: bs_shape refuses anything else.
// All stores are ordinary vector stores; every index read from an array is clamped to its table before it forms an address.
#include <cstring>  // rocprim 4.x headers use memset without including it
#include <rocprim/rocprim.hpp>

#include "cgcn_compact.hpp"

#define BS_THREADS 256
#define BS_BATCH 16   // row loads in flight per lane of the walk
#define BS_SEG 64     // rows per wave of the sliding sum: at least, and
#define BS_SEG_MAX 4096   // at most
#define BS_IDX_MASK 0x3FFFFFFFu
#define BS_TARGET 0x40000000u
#define BS_END 0x80000000u

// key(seed, b, 5) of the rule: dropout_key with the step counter replaced by the replicate's absolute index (64 bits)
__device__ __forceinline__ uint32_t bs_key(u64 seed, u64 b) {
  uint32_t k = mix32((uint32_t)seed ^ 0x9E3779B9u);
  k = mix32(k ^ (uint32_t)(seed >> 32));
  k = mix32(k + (uint32_t)b * 0x85EBCA6Bu);
  return mix32(k ^ (uint32_t)(b >> 32) ^ (5u * 0xC2B2AE35u));
}

// ---------------------------------------------------------------------------------------------------------------------
// the sort
// [n, C] row-major -> keys[c * n + i], transposed through LDS so that both sides are coalesced.  A NaN score sets bad.
__global__ __launch_bounds__(BS_THREADS) void k_bs_pack(long long n, int C, int bN, const float* __restrict__ probs,
                                                        const float* __restrict__ targets, u64* __restrict__ keys,
                                                        int* __restrict__ bad) {
  __shared__ float tp[32][33];
  __shared__ float tt[32][33];
  const long long i0 = (long long)blockIdx.x * 32;
  const int c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    const long long i = i0 + r;
    const int c = c0 + tx;
    const bool ok = i < n && c < C;
    tp[r][tx] = ok ? probs[i * C + c] : 0.f;
    tt[r][tx] = ok ? targets[i * C + c] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int c = c0 + r;
    const long long i = i0 + tx;
    if (c < C && i < n) {
      const float s = tp[tx][r];
      if (s != s) atomicOr(bad, 1);
      unsigned u = __float_as_uint(s == 0.f ? 0.f : s);   // -0 is folded onto +0
      u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
      keys[(long long)c * n + i] = ((u64)(unsigned)c << (33 + bN)) | ((u64)(~u) << (1 + bN)) |
                                   ((tt[tx][r] > 0.5f ? 1ull : 0ull) << bN) | (u64)i;
    }
  }
}

// sorted keys -> one word per element: window index | target << 30 | run end << 31
__global__ __launch_bounds__(BS_THREADS) void k_bs_order(long long n, long long items, int bN, const u64* __restrict__ sorted,
                                                         unsigned* __restrict__ order) {
  const long long j = (long long)blockIdx.x * BS_THREADS + threadIdx.x;
  if (j >= items) return;
  const u64 k = sorted[j];
  bool end = j % n == n - 1;
  if (!end) end = (sorted[j + 1] >> (1 + bN)) != (k >> (1 + bN));   // another (label, score)
  long long idx = (long long)(k & ((1ull << bN) - 1ull));
  if (idx >= n) idx = n - 1;
  order[j] = (unsigned)idx | (((k >> bN) & 1ull) ? BS_TARGET : 0u) | (end ? BS_END : 0u);
}

// ---------------------------------------------------------------------------------------------------------------------
// the weights
// One thread per (draw g, replicate r): the stratum of g by a walk over the offsets, then one integer atomic.
__global__ __launch_bounds__(BS_THREADS) void k_bs_starts(long long n, u64 rep0, int R, int n_strata,
                                                          const int* __restrict__ offsets, int block, long long draws, u64 seed,
                                                          int* __restrict__ hist, int* __restrict__ flags) {
  const long long g = (long long)blockIdx.x * BS_THREADS + threadIdx.x;
  const int r = blockIdx.y;
  if (g >= draws || r >= R) return;
  long long base = 0;
  for (int s = 0; s < n_strata; ++s) {
    const long long lo = offsets[s], hi = offsets[s + 1];
    if (lo < 0 || hi < lo || hi > n) {
      atomicOr(flags, CGCN_BOOT_FLAG_STRATA);
      return;
    }
    const long long ns = hi - lo;
    if (ns == 0) continue;
    const long long L = block < ns ? block : ns;
    const long long k = (ns + L - 1) / L;
    if (g < base + k) {
      const uint32_t start = (uint32_t)(((u64)mix32((uint32_t)g * 0x9E3779B1u + bs_key(seed, rep0 + (u64)r)) * (u64)ns) >> 32);
      atomicAdd(&hist[((long long)(r >> 6) * n + lo + start) * WAVE + (r & 63)], 1);
      return;
    }
    base += k;
  }
}

// The circular sliding sum: a wave takes `seg` consecutive rows of one group, lane = replicate.  The window sum is formed
// anew (L_s reads) at the wave's first row and at every stratum's first row, and slid by one row (two reads) otherwise; the
// host passes seg = block clamped to [BS_SEG, BS_SEG_MAX], so that up to a block of 4096 a wave never spends more on forming
// sums than on sliding them (at most three histogram reads per row) while a chromosome still gives every group dozens of
// waves; a longer block costs 2 + L_s / 4096 reads per row.  A stratum that is one block (L_s = n_s: one draw) needs no read:
// every row of a replicate has weight 1.
__global__ __launch_bounds__(BS_THREADS) void k_bs_slide(long long n, int R, int n_strata, const int* __restrict__ offsets, int block,
                                                         long long seg, const int* __restrict__ hist,
                                                         unsigned char* __restrict__ tile, int* __restrict__ flags) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long long i0 = ((long long)blockIdx.x * (BS_THREADS / WAVE) + threadIdx.x / WAVE) * seg;
  const int whole = (int)blockIdx.y * WAVE + lane < R ? 1 : 0;
  const long long gbase = (long long)blockIdx.y * n;
  int s = 0, over = 0;
  int sum = 0;
  bool fresh = true;
  for (long long i = i0; i < i0 + seg && i < n; ++i) {
    while (s < n_strata && i >= offsets[s + 1]) {
      ++s;
      fresh = true;
    }
    long long lo = 0, hi = 0;
    if (s < n_strata) {
      lo = offsets[s];
      hi = offsets[s + 1];
    }
    int w = 0;
    if (lo >= 0 && lo <= i && i < hi && hi <= n) {   // (rows outside every stratum keep weight 0)
      const long long ns = hi - lo;
      const long long L = block < ns ? block : ns;
      if (L == ns) {
        sum = whole;
        fresh = true;
      } else if (fresh || i == lo) {
        sum = 0;
        long long p = i - lo;
        for (long long q = 0; q < L; ++q) {
          sum += hist[(gbase + lo + p) * WAVE + lane];
          p = p == 0 ? ns - 1 : p - 1;
        }
        fresh = false;
      } else {
        long long p = i - lo - L;
        if (p < 0) p += ns;
        sum += hist[(gbase + i) * WAVE + lane] - hist[(gbase + lo + p) * WAVE + lane];
      }
      w = sum;
    }
    if (w > 255) over = 1;
    tile[(gbase + i) * WAVE + lane] = (unsigned char)w;
  }
  if (over) atomicOr(flags, CGCN_BOOT_FLAG_WEIGHT);
}

// explicit weights int32 [R, n] -> the tile, 64 windows x 64 replicates per workgroup through LDS
__global__ __launch_bounds__(BS_THREADS) void k_bs_weights_in(long long n, int R, const int* __restrict__ weights,
                                                              unsigned char* __restrict__ tile, int* __restrict__ flags) {
  __shared__ int t[WAVE][WAVE + 1];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const long long i0 = (long long)blockIdx.x * WAVE;
  const int r0 = blockIdx.y * WAVE;
  int bad = 0;
  for (int rr = wave; rr < WAVE; rr += BS_THREADS / WAVE) {
    const int r = r0 + rr;
    const long long i = i0 + lane;
    int v = 0;
    if (r < R && i < n) v = weights[(long long)r * n + i];
    if (v < 0) {
      bad |= CGCN_BOOT_FLAG_NEGATIVE;
      v = 0;
    }
    if (v > 255) bad |= CGCN_BOOT_FLAG_WEIGHT;
    t[rr][lane] = v;
  }
  __syncthreads();
  for (int ii = wave; ii < WAVE; ii += BS_THREADS / WAVE) {
    const long long i = i0 + ii;
    if (i < n) tile[((long long)blockIdx.y * n + i) * WAVE + lane] = (unsigned char)t[lane][ii];
  }
  if (bad) atomicOr(flags, bad);
}

// ---------------------------------------------------------------------------------------------------------------------
// the walk
struct BsLane {
  unsigned tp, tot, ptp, pfp;   // running sums of w t and w; tp and fp of the previous point
  double pp, sap, spr;          // p of the previous point; the two float64 sums
  u64 A;
  unsigned F;
};

__device__ __forceinline__ void bs_point(BsLane& s, double q) {
  if (s.tot == 0u) return;   // a leading run without weight is no curve point
  const unsigned fp = s.tot - s.tp;
  const double p = (double)s.tp / (double)s.tot;
  const double dtp = (double)(s.tp - s.ptp);
  s.A += (u64)(fp - s.pfp) * (u64)(s.tp + s.ptp);
  s.sap += dtp * p;
  s.spr += dtp * (p + s.pp);
  if ((double)fp <= q * (double)s.tot) s.F = s.tp;
  s.ptp = s.tp;
  s.pfp = fp;
  s.pp = p;
}

__global__ __launch_bounds__(WAVE) void k_bs_walk(long long n, int C, int R, const unsigned* __restrict__ order,
                                                  const unsigned char* __restrict__ tile, double q, long long* __restrict__ out) {
  const int lane = threadIdx.x;
  const int c = blockIdx.x % C, g = blockIdx.x / C;   // the labels of one group run together: they share its tile
  const unsigned* __restrict__ list = order + (long long)c * n;
  const unsigned char* __restrict__ rows = tile + (long long)g * n * WAVE + lane;
  BsLane s = {0u, 0u, 0u, 0u, 1.0, 0.0, 0.0, 0ull, 0u};
  for (long long k0 = 0; k0 < n; k0 += WAVE) {
    const int cnt = (int)(n - k0 < WAVE ? n - k0 : WAVE);
    const unsigned ev = lane < cnt ? list[k0 + lane] : 0u;
#pragma unroll
    for (int u0 = 0; u0 < WAVE; u0 += BS_BATCH) {
      if (u0 >= cnt) break;
      unsigned e[BS_BATCH];
      unsigned char w[BS_BATCH];
#pragma unroll
      for (int u = 0; u < BS_BATCH; ++u) {
        e[u] = (unsigned)__builtin_amdgcn_readlane((int)ev, u0 + u);
        long long idx = (long long)(e[u] & BS_IDX_MASK);
        if (idx >= n) idx = n - 1;
        w[u] = rows[idx * WAVE];   // (behind the list: window 0, unused)
      }
#pragma unroll
      for (int u = 0; u < BS_BATCH; ++u) {
        if (u0 + u < cnt) {
          s.tot += w[u];
          if (e[u] & BS_TARGET) s.tp += w[u];
          if (e[u] & BS_END) bs_point(s, q);
        }
      }
    }
  }
  const int r = g * WAVE + lane;
  if (r < R) {
    const long long RC = (long long)R * C, at = (long long)r * C + c;
    out[at] = (long long)s.A;
    out[RC + at] = (long long)s.tp;
    out[2 * RC + at] = (long long)s.tot;
    out[3 * RC + at] = (long long)s.F;
    ((double*)out)[4 * RC + at] = s.sap;
    ((double*)out)[5 * RC + at] = s.spr;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
struct BsPlan {
  int bN;
  unsigned bits;
  size_t temp, o_keyA, o_keyB, o_temp, sort_total, hist_bytes, total;
};

static bool bs_shape(long long n, int C) { return n >= 1 && C >= 1 && n < (1ll << 23) && C <= (1 << 20) && n * C <= (1ll << 31); }

static bool bs_plan(long long n, int C, int R, BsPlan* p) {
  if (!bs_shape(n, C) || R < 0 || R > (1 << 20)) return false;
  p->bN = bits_for(n);
  const int bits = bits_for(C) + 33 + p->bN;
  if (bits > 64) return false;
  p->bits = (unsigned)bits;
  p->temp = 0;
  (void)rocprim::radix_sort_keys(nullptr, p->temp, (const u64*)nullptr, (u64*)nullptr, (size_t)(n * C), 0u, p->bits);
  WsBump b = {0};
  p->o_keyA = b.take((size_t)(n * C) * 8);
  p->o_keyB = b.take((size_t)(n * C) * 8);
  p->o_temp = b.take(p->temp);
  p->sort_total = b.o + 256;
  p->hist_bytes = (size_t)tiles_of(R, WAVE) * (size_t)n * WAVE * 4;
  p->total = R > 0 ? ws_align(p->hist_bytes) + 256 : 0;
  if (p->sort_total > p->total) p->total = p->sort_total;
  return true;
}

extern "C" {

size_t cgcn_bootstrap_workspace_bytes(long long n, int C, int R) {
  BsPlan p;
  return bs_plan(n, C, R, &p) ? p.total : 0;
}

int cgcn_bootstrap_sort(cgcn_stream_t stream, long long n, int C, const float* probs, const float* targets, uint32_t* order,
                        int32_t* bad, void* workspace, size_t workspace_bytes) {
  BsPlan p;
  if (!bs_plan(n, C, 0, &p)) return n < 0 || C < 0 ? CGCN_ERR_BAD_ARG : CGCN_ERR_UNSUPPORTED;
  if (!probs || !targets || !order || !bad || !workspace) return CGCN_ERR_BAD_ARG;
  if (workspace_bytes < p.sort_total) return CGCN_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* w = ws_base(workspace);
  u64* keyA = (u64*)(w + p.o_keyA);
  u64* keyB = (u64*)(w + p.o_keyB);
  const long long items = n * C;
  hipLaunchKernelGGL(k_bs_pack, dim3((unsigned)tiles_of(n, 32), (unsigned)tiles_of(C, 32)), dim3(BS_THREADS), 0, st, n, C, p.bN, probs,
                     targets, keyA, (int*)bad);
  size_t temp = p.temp;
  if (rocprim::radix_sort_keys((void*)(w + p.o_temp), temp, (const u64*)keyA, keyB, (size_t)items, 0u, p.bits, st) != hipSuccess)
    return CGCN_ERR_LAUNCH;
  hipLaunchKernelGGL(k_bs_order, dim3((unsigned)tiles_of(items, BS_THREADS)), dim3(BS_THREADS), 0, st, n, items, p.bN, (const u64*)keyB,
                     (unsigned*)order);
  return launch_status();
}

int cgcn_bootstrap_weights(cgcn_stream_t stream, long long n, long long rep0, int R, int n_strata, const int32_t* offsets, int block,
                           long long draws, long long seed, unsigned char* tile, int32_t* flags, void* workspace,
                           size_t workspace_bytes) {
  if (n < 0 || R < 1 || n_strata < 1 || block < 1 || draws < 0) return CGCN_ERR_BAD_ARG;
  BsPlan p;
  if (!bs_plan(n, 1, R, &p) || draws >= (1ll << 31) || R > 65535) return CGCN_ERR_UNSUPPORTED;
  if (!offsets || !tile || !flags || !workspace) return CGCN_ERR_BAD_ARG;
  if (workspace_bytes < ws_align(p.hist_bytes) + 256) return CGCN_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  int* hist = (int*)ws_base(workspace);
  const unsigned G = (unsigned)tiles_of(R, WAVE);
  if (hipMemsetAsync(hist, 0, p.hist_bytes, st) != hipSuccess) return CGCN_ERR_LAUNCH;
  if (draws > 0)
    hipLaunchKernelGGL(k_bs_starts, dim3((unsigned)tiles_of(draws, BS_THREADS), (unsigned)R), dim3(BS_THREADS), 0, st, n, (u64)rep0, R,
                       n_strata, (const int*)offsets, block, draws, (u64)seed, hist, (int*)flags);
  const long long seg = block < BS_SEG ? BS_SEG : (block > BS_SEG_MAX ? BS_SEG_MAX : block);
  hipLaunchKernelGGL(k_bs_slide, dim3((unsigned)tiles_of(n, seg * (BS_THREADS / WAVE)), G), dim3(BS_THREADS), 0, st, n, R, n_strata,
                     (const int*)offsets, block, seg, (const int*)hist, tile, (int*)flags);
  return launch_status();
}

int cgcn_bootstrap_weights_in(cgcn_stream_t stream, long long n, int R, const int32_t* weights, unsigned char* tile, int32_t* flags) {
  if (n < 0 || R < 1) return CGCN_ERR_BAD_ARG;
  if (!bs_shape(n, 1) || R > 65535 * WAVE) return CGCN_ERR_UNSUPPORTED;
  if (!weights || !tile || !flags) return CGCN_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_bs_weights_in, dim3((unsigned)tiles_of(n, WAVE), (unsigned)tiles_of(R, WAVE)), dim3(BS_THREADS), 0,
                     (hipStream_t)stream, n, R, (const int*)weights, tile, (int*)flags);
  return launch_status();
}

int cgcn_bootstrap_sums(cgcn_stream_t stream, long long n, int C, int R, const uint32_t* order, const unsigned char* tile,
                        const double* fdr_cutoff, long long* out) {
  if (n < 0 || C < 0 || R < 1) return CGCN_ERR_BAD_ARG;
  if (!bs_shape(n, C) || tiles_of(R, WAVE) * C >= (1ll << 31)) return CGCN_ERR_UNSUPPORTED;
  if (!order || !tile || !fdr_cutoff || !out) return CGCN_ERR_BAD_ARG;
  const double q = *fdr_cutoff;
  if (!(q > 0.0 && q < 1.0)) return CGCN_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_bs_walk, dim3((unsigned)(tiles_of(R, WAVE) * C)), dim3(WAVE), 0, (hipStream_t)stream, n, C, R,
                     (const unsigned*)order, tile, q, out);
  return launch_status();
}

}  // extern "C"
