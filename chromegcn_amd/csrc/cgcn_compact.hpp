// chromegcn_amd/csrc/cgcn_compact.hpp
//
// The pieces of an ordered count / scan / write pass, in one place for every ingest unit:
//   k_tile_scan          exclusive scan of the per-tile counts, one workgroup
//   lines_*              the line-start front end of the text parsers (cgcn_text.hip, cgcn_pairs.hip)
//   wave_excl_sum, wg_count, wg_before, WgFlags   a thread's rank among the flagged threads (or counted items) of a workgroup
//   ws_align, ws_base, WsBump, bits_for, tiles_of   host side: the workspace layout and the sizes of a plan
// Everything here is a template, an inline function or static: a unit that includes the header gets its own instances,
// the k_tile_scan kernel included (as with the rocprim::radix_sort_keys<u64> kernels of the same units).
#pragma once
#include "cgcn_common.hpp"

typedef unsigned long long u64;

// exclusive scan of counts[0..nb) into off[0..nb); the total goes to total64[0] and, clamped to `clamp`, to total32[0]
// (either may be NULL).  One workgroup of 1024 threads: launch as k_tile_scan<>.
template <int UNIT = 0>
__global__ __launch_bounds__(1024) void k_tile_scan(int nb, const int* __restrict__ counts, long long* __restrict__ off,
                                                    long long* __restrict__ total64, int* __restrict__ total32, long long clamp) {
  __shared__ long long part[1024];
  const int t = threadIdx.x;
  const int per = (nb + 1023) / 1024;
  const int i0 = min(nb, t * per), i1 = min(nb, i0 + per);
  long long s = 0;
  for (int i = i0; i < i1; ++i) s += counts[i];
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const long long v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  long long run = t ? part[t - 1] : 0;
  for (int i = i0; i < i1; ++i) {
    off[i] = run;
    run += counts[i];
  }
  if (t == 1023) {
    const long long tot = part[1023];
    if (total64) total64[0] = tot;
    if (total32) total32[0] = (int)(tot < clamp ? tot : clamp);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Ranks inside a workgroup.  Every wave leaves its count in wave_tot[wave]; behind the barrier a thread's rank is (lanes
// before) + (waves before), and the sum of wave_tot[] is the workgroup's count.

// sum of `c` over the lanes before this one (all 64 lanes active)
__device__ __forceinline__ int wave_excl_sum(int c, int lane) {
  int inc = c;
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const int t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  return inc - c;
}

// the workgroup's count (WAVES waves)
template <int WAVES = 4>
__device__ __forceinline__ int wg_count(const int* wave_tot) {
  int s = wave_tot[0];
#pragma unroll
  for (int k = 1; k < WAVES; ++k) s += wave_tot[k];
  return s;
}

// r (a base plus the count of the lanes before) plus the counts of the waves before
template <class T>
__device__ __forceinline__ T wg_before(T r, const int* wave_tot) {
  const int w = threadIdx.x / WAVE;
  for (int k = 0; k < w; ++k) r += wave_tot[k];
  return r;
}

// One flag per thread: the ballot, the wave's count into wave_tot[] and the barrier.  Every thread of the workgroup
// constructs it.
template <int WAVES = 4>
struct WgFlags {
  u64 m;
  const int* wave_tot;
  __device__ __forceinline__ WgFlags(bool flag, int* wave_tot_) : m(__ballot(flag)), wave_tot(wave_tot_) {
    if ((threadIdx.x & (WAVE - 1)) == 0) wave_tot_[threadIdx.x / WAVE] = __popcll(m);
    __syncthreads();
  }
  __device__ __forceinline__ int count() const { return wg_count<WAVES>(wave_tot); }
  // base + the flagged threads before this one
  template <class T>
  __device__ __forceinline__ T before(T base) const {
    return wg_before(base + __popcll(m & ((1ull << (threadIdx.x & (WAVE - 1))) - 1ull)), wave_tot);
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// Line starts of a text: 256 threads, 16 bytes per lane, 4 KiB per workgroup.
#define LINES_THREADS 256
#define LINES_CHUNK 16                                 // bytes per lane
#define LINES_TILE (LINES_THREADS * LINES_CHUNK)       // bytes per workgroup

// the 16 bytes at g (g a multiple of 16, g < n); bytes at or behind n read as 0.  The text base is 16-byte aligned.
__device__ __forceinline__ u32x4 lines_load16(const unsigned char* __restrict__ text, long long n, long long g) {
  if (g + LINES_CHUNK <= n) return *(const u32x4*)(text + g);
  u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < LINES_CHUNK; ++k)
    if (g + k < n) v[k >> 2] |= (uint32_t)text[g + k] << ((k & 3) * 8);
  return v;
}

// bit k: byte g + k starts a line (it exists, and it is byte 0 or follows an LF)
__device__ __forceinline__ unsigned lines_start_mask(const u32x4 v, bool after_lf, long long n, long long g) {
  unsigned lf = 0;
#pragma unroll
  for (int k = 0; k < LINES_CHUNK; ++k) lf |= (((v[k >> 2] >> ((k & 3) * 8)) & 0xFFu) == 0x0Au ? 1u : 0u) << k;
  const unsigned starts = ((lf << 1) | (after_lf ? 1u : 0u)) & 0xFFFFu;
  const long long left = n - g;
  return left >= LINES_CHUNK ? starts : (left <= 0 ? 0u : starts & ((1u << (int)left) - 1u));
}

struct LinesFront {
  u32x4 v;           // the lane's 16 bytes
  unsigned starts;   // their start mask
  int before;        // line starts in the lanes before it (of its wave)
};

// The opening of a pass over tile blockIdx.x: the lane's 16 bytes and their start mask, and the wave's count into
// wave_tot[wave].  The caller's __syncthreads() follows; behind it wg_count(wave_tot) is the tile's line count and
// wg_before(base + before, wave_tot) the index of the lane's first line.  (A caller that parses stages v and the bytes
// behind the tile into LDS before its barrier.  That staging is not in here: wrapped in a function it reorders the
// instructions of k_pairs_starts<true>.)
__device__ __forceinline__ LinesFront lines_tile_front(const unsigned char* __restrict__ text, long long n, int* wave_tot) {
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  const long long g = (long long)blockIdx.x * LINES_TILE + (long long)threadIdx.x * LINES_CHUNK;
  LinesFront f;
  f.v = u32x4{0u, 0u, 0u, 0u};
  bool after_lf = false;
  if (g < n) {
    f.v = lines_load16(text, n, g);
    after_lf = g == 0 || text[g - 1] == 0x0Au;
  }
  f.starts = lines_start_mask(f.v, after_lf, n, g);
  const int mine = __popc(f.starts);
  f.before = wave_excl_sum(mine, lane);
  if (lane == WAVE - 1) wave_tot[w] = f.before + mine;
  return f;
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side.  A workspace is laid out from a base rounded up to 256 bytes, every buffer at a multiple of 256 bytes: a plan's
// total is the buffers' sum + 256 for the rounding.
static inline size_t ws_align(size_t x) { return (x + 255) & ~(size_t)255; }
static inline char* ws_base(void* workspace) { return (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255); }

// the offset of the next buffer of `bytes` bytes
struct WsBump {
  size_t o;
  size_t take(size_t bytes) {
    const size_t at = o;
    o += ws_align(bytes);
    return at;
  }
};

// bits of an index below n: 1 .. 31
static inline int bits_for(long long n) {
  int b = 1;
  while (b < 31 && (1ll << b) < n) ++b;
  return b;
}
// tiles of `tile` items over n items, at least one
static inline long long tiles_of(long long n, long long tile) {
  const long long k = (n + tile - 1) / tile;
  return k < 1 ? 1 : k;
}
