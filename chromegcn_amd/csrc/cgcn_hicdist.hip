// chromegcn_amd/csrc/cgcn_hicdist.hip
//
// Distance sums of one chromosome's contact records (chromegcn_amd/hicdist.py holds the definitions
// and their numpy restatement): raw[d] = sum of count and act[d] = sum of count / (nv[b1] nv[b2]) over the records whose two
// bins are d apart, the input of the expected vector.
//
//   k_hd_keys            one pass over the M records: the 64-bit key (d << rb | record), rb = bits of M; a record with a bad
//                        count, a negative position or a bin outside n_bins gets the pad distance n_bins instead and raises a
//                        flag; the largest bin + 1
//   rocprim::radix_sort_keys    keys alone (the pair sort of rocprim 4 uses scratch memory on gfx950, see cgcn_hicnorm.hip):
//                        the records of one distance come out together, in record order
//   k_hd_tiles           a wavefront owns 64 consecutive sorted keys: every lane fetches its record and computes the two
//                        values once; a segmented scan over the lanes (six shuffle steps whose shape depends on the keys
//                        alone) leaves every run's sums in its last lane.  A run that touches neither end of the tile is a
//                        whole distance and is written; the run at the tile's start and the run at its end leave as the
//                        tile's two partials
//   k_hd_fold            one wavefront per distance: the bounds of its run by binary search; lane l adds the partials of the
//                        run's tiles l, l + 64, ... in tile order, then one fixed butterfly over the lanes
// No floating-point atomic, no order that scheduling could change: the same bits in every run, and exact sums for integer
// counts below 2^53.  Nothing is allocated, nothing synchronises.
#include <cstring>  // rocprim 4.x headers use memset without including it
#include <rocprim/rocprim.hpp>

#include "cgcn_compact.hpp"
#include "cgcn_hicmap.hpp"

#define HD_THREADS 256
#define HD_NONE 0xFFFFFFFFu                            // no distance: the lanes behind the last key, a tile without a second partial

static inline int hd_bits(long long n) {
  int b = 1;
  while (b < 32 && (1ll << b) < n) ++b;
  return b;
}

// sizes[0] |= 1: a count that is negative or not finite; |= 2: a negative position; |= 4: a bin >= n_bins (n_bins > 0).
// sizes[1] = the largest bin + 1 of the records with positions >= 0.  keys == NULL: the flags and the bins alone.
__global__ __launch_bounds__(HD_THREADS) void k_hd_keys(long long M, const int* __restrict__ pos1, const int* __restrict__ pos2,
                                                        const double* __restrict__ count, int res, long long n_bins, int rb,
                                                        u64* __restrict__ keys, u64* sizes) {
  __shared__ unsigned wave_top[HD_THREADS / WAVE];
  const long long r = (long long)blockIdx.x * HD_THREADS + threadIdx.x;
  unsigned bad = 0;
  long long top = 0;
  if (r < M) {
    const int a = pos1[r], c = pos2[r];
    const double v = count[r];
    long long d = n_bins;
    bad = (v >= 0.0 && v < hm_inf()) ? 0u : 1u;
    if (a < 0 || c < 0) {
      bad |= 2u;
    } else {
      const long long i = a / res, j = c / res;
      top = (i > j ? i : j) + 1;
      if (n_bins > 0 && top > n_bins) bad |= 4u;
      else if (!bad) d = i > j ? i - j : j - i;
    }
    if (keys) keys[r] = ((u64)d << rb) | (u64)r;
  }
  unsigned wtop = (unsigned)top;
#pragma unroll
  for (int o = WAVE / 2; o >= 1; o >>= 1) wtop = max(wtop, (unsigned)__shfl_xor((int)wtop, o));
  if ((threadIdx.x & (WAVE - 1)) == 0) wave_top[threadIdx.x / WAVE] = wtop;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned g = max(max(wave_top[0], wave_top[1]), max(wave_top[2], wave_top[3]));
    if ((u64)g > __atomic_load_n(&sizes[1], __ATOMIC_RELAXED)) atomicMax(&sizes[1], (u64)g);
  }
  if (bad) atomicOr(&sizes[0], (u64)bad);
}

// tile t = sorted keys [64 t, 64 t + 64).  tile_key[2 t], tile_sum[4 t .. 4 t + 1]: the distance and the (raw, act) sums of
// the run at the tile's start; [2 t + 1], [4 t + 2 .. 4 t + 3]: of the run at its end, HD_NONE when that is the same run.
__global__ __launch_bounds__(HD_THREADS) void k_hd_tiles(long long M, const u64* __restrict__ keys, int rb,
                                                         const int* __restrict__ pos1, const int* __restrict__ pos2,
                                                         const double* __restrict__ count, const double* __restrict__ norm,
                                                         long long n_norm, int res, long long n_bins, unsigned* __restrict__ tile_key,
                                                         double* __restrict__ tile_sum, double* __restrict__ raw_out,
                                                         double* __restrict__ act_out) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long long t = (long long)blockIdx.x * (HD_THREADS / WAVE) + threadIdx.x / WAVE;
  if (t * WAVE >= M) return;   // the whole wavefront
  const long long e = t * WAVE + lane;
  unsigned d = HD_NONE;
  double raw = 0.0, act = 0.0;
  if (e < M) {
    const u64 key = keys[e];
    d = (unsigned)(key >> rb);
    if ((long long)d < n_bins) {   // no pad
      const long long r = (long long)(key & ((1ull << rb) - 1ull));
      raw = act = count[r];
      if (norm) {
        const double den = hm_norm_at(norm, n_norm, pos1[r] / res) * hm_norm_at(norm, n_norm, pos2[r] / res);   // positions >= 0
        act = raw / den;   // one multiply, one divide; a NaN or 0 norm bin: the record adds 0
      }
    }
  }
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const unsigned ud = (unsigned)__shfl_up((int)d, o);
    const double ur = __shfl_up(raw, o), ua = __shfl_up(act, o);
    if (lane >= o && ud == d) {   // sorted: equal ends mean one run
      raw = ur + raw;
      act = ua + act;
    }
  }
  const unsigned first = (unsigned)__shfl((int)d, 0), last = (unsigned)__shfl((int)d, WAVE - 1);
  const unsigned next = (unsigned)__shfl_down((int)d, 1);
  const bool tail = lane == WAVE - 1 || next != d;
  if (lane == 0 && (first == last || last == HD_NONE)) tile_key[2 * t + 1] = HD_NONE;   // no run at the tile's end
  if (!tail || d == HD_NONE) return;
  if (d == first) {
    tile_key[2 * t] = d;
    tile_sum[4 * t] = raw;
    tile_sum[4 * t + 1] = act;
  } else if (d == last) {
    tile_key[2 * t + 1] = d;
    tile_sum[4 * t + 2] = raw;
    tile_sum[4 * t + 3] = act;
  } else if ((long long)d < n_bins) {
    raw_out[d] = raw;
    act_out[d] = act;
  }
}

// The double shuffle in two explicit halves: with HIP's own overload (wave_sum_d) k_hd_fold's two butterflies compile to
// another block layout, and the one run that timed it had chr21's distance sums at 0.532 ms against 0.519 / 0.520 ms before.
// One run is not proof, but nothing speaks for the change either: this one kernel keeps the code it had.
__device__ __forceinline__ double hd_shfl_xor(double v, int o) {
  const long long x = __double_as_longlong(v);
  const int lo = __shfl_xor((int)(x & 0xFFFFFFFFll), o), hi = __shfl_xor((int)(x >> 32), o);
  return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

// first index of keys[0..M) whose distance is >= d
__device__ __forceinline__ long long hd_lower(const u64* __restrict__ keys, long long M, int rb, u64 d) {
  long long lo = 0, hi = M;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if ((keys[mid] >> rb) < d) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(HD_THREADS) void k_hd_fold(long long M, const u64* __restrict__ keys, int rb, long long n_bins,
                                                        const unsigned* __restrict__ tile_key, const double* __restrict__ tile_sum,
                                                        double* __restrict__ raw_out, double* __restrict__ act_out) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long long d = (long long)blockIdx.x * (HD_THREADS / WAVE) + threadIdx.x / WAVE;
  if (d >= n_bins) return;   // the whole wavefront
  const long long s = hd_lower(keys, M, rb, (u64)d), e = hd_lower(keys, M, rb, (u64)d + 1);
  if (s == e) {
    if (lane == 0) raw_out[d] = act_out[d] = 0.0;
    return;
  }
  const long long t0 = s / WAVE, t1 = (e - 1) / WAVE;
  // inside one tile and at neither of its ends: k_hd_tiles wrote it (a run that ends at M inside the last tile is followed
  // by lanes without a key: it is no run at the tile's end)
  if (t0 == t1 && (s % WAVE) != 0 && (e % WAVE) != 0) return;
  double raw = 0.0, act = 0.0;
  for (long long t = t0 + lane; t <= t1; t += WAVE) {
    if (tile_key[2 * t] == (unsigned)d) {
      raw += tile_sum[4 * t];
      act += tile_sum[4 * t + 1];
    }
    if (tile_key[2 * t + 1] == (unsigned)d) {
      raw += tile_sum[4 * t + 2];
      act += tile_sum[4 * t + 3];
    }
  }
#pragma unroll
  for (int o = WAVE / 2; o >= 1; o >>= 1) {   // the two butterflies step by step: their shuffles share one wait
    raw += hd_shfl_xor(raw, o);
    act += hd_shfl_xor(act, o);
  }
  if (lane == 0) {
    raw_out[d] = raw;
    act_out[d] = act;
  }
}

struct HdPlan {
  int rb, bits;
  long long tiles;
  size_t temp, o_keyA, o_keyB, o_tkey, o_tsum, o_temp, total;
};

static bool hd_plan(long long M, long long n_bins, HdPlan* p) {
  if (M < 0 || n_bins < 0 || M >= 2147483648ll || n_bins >= 2147483647ll) return false;
  p->rb = hd_bits(M);
  p->bits = p->rb + hd_bits(n_bins + 1);
  p->tiles = tiles_of(M, WAVE);
  p->temp = 0;
  WsBump w = {0};
  p->o_keyA = p->o_keyB = p->o_tkey = p->o_tsum = p->o_temp = 0;
  if (n_bins > 0) {
    const size_t m = (size_t)(M < 1 ? 1 : M);
    (void)rocprim::radix_sort_keys(nullptr, p->temp, (const u64*)nullptr, (u64*)nullptr, m, 0u, (unsigned)p->bits);
    p->o_keyA = w.take(m * 8);
    p->o_keyB = w.take(m * 8);
    p->o_tkey = w.take((size_t)p->tiles * 8);
    p->o_tsum = w.take((size_t)p->tiles * 32);
    p->o_temp = w.take(p->temp);
  }
  p->total = w.o + 256;   // the base is rounded up to 256 bytes
  return true;
}

extern "C" {

size_t cgcn_hicdist_workspace_bytes(long long M, long long n_bins) {
  HdPlan p;
  return hd_plan(M, n_bins, &p) ? p.total : 0;
}

int cgcn_hicdist_sums(cgcn_stream_t stream, long long M, const int32_t* pos1, const int32_t* pos2, const double* count,
                      const double* norm, long long n_norm, int resolution_bp, long long n_bins, void* workspace,
                      size_t workspace_bytes, double* raw_out, double* act_out, unsigned long long* sizes) {
  if (M < 0 || n_bins < 0 || n_norm < 0 || resolution_bp < 1 || !sizes || !workspace) return CGCN_ERR_BAD_ARG;
  if (M > 0 && (!pos1 || !pos2 || !count)) return CGCN_ERR_BAD_ARG;
  if (n_bins > 0 && (!raw_out || !act_out)) return CGCN_ERR_BAD_ARG;
  if (norm && n_norm < 1) return CGCN_ERR_BAD_ARG;
  HdPlan p;
  if (!hd_plan(M, n_bins, &p)) return CGCN_ERR_UNSUPPORTED;
  if (workspace_bytes < p.total) return CGCN_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(sizes, 0, 16, st) != hipSuccess) return CGCN_ERR_LAUNCH;
  if (M == 0) {
    if (n_bins > 0 && (hipMemsetAsync(raw_out, 0, (size_t)n_bins * 8, st) != hipSuccess ||
                       hipMemsetAsync(act_out, 0, (size_t)n_bins * 8, st) != hipSuccess))
      return CGCN_ERR_LAUNCH;
    return CGCN_OK;
  }
  char* w = ws_base(workspace);
  u64* keyA = (u64*)(w + p.o_keyA);
  u64* keyB = (u64*)(w + p.o_keyB);
  const unsigned blocksM = (unsigned)tiles_of(M, HD_THREADS);
  hipLaunchKernelGGL(k_hd_keys, dim3(blocksM), dim3(HD_THREADS), 0, st, M, pos1, pos2, count, resolution_bp, n_bins, p.rb,
                     n_bins > 0 ? keyA : (u64*)nullptr, (u64*)sizes);
  if (n_bins == 0) return launch_status();
  size_t temp = p.temp;
  if (rocprim::radix_sort_keys((void*)(w + p.o_temp), temp, (const u64*)keyA, keyB, (size_t)M, 0u, (unsigned)p.bits, st) != hipSuccess)
    return CGCN_ERR_LAUNCH;
  unsigned* tkey = (unsigned*)(w + p.o_tkey);
  double* tsum = (double*)(w + p.o_tsum);
  hipLaunchKernelGGL(k_hd_tiles, dim3((unsigned)tiles_of(p.tiles, HD_THREADS / WAVE)), dim3(HD_THREADS), 0, st, M, (const u64*)keyB,
                     p.rb, pos1, pos2, count, norm, n_norm, resolution_bp, n_bins, tkey, tsum, raw_out, act_out);
  hipLaunchKernelGGL(k_hd_fold, dim3((unsigned)tiles_of(n_bins, HD_THREADS / WAVE)), dim3(HD_THREADS), 0, st, M, (const u64*)keyB, p.rb,
                     n_bins, (const unsigned*)tkey, (const double*)tsum, raw_out, act_out);
  return launch_status();
}

}  // extern "C"
