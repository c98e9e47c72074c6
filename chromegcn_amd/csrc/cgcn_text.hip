// chromegcn_amd/csrc/cgcn_text.hip
//
// Hi-C contact text (`RAWobserved`: pos1<TAB>pos2<TAB>count per line) parsed on the device into the arrays HicContacts holds
// (the rule is stated once in include/chromegcn.h above cgcn_text_count).
//
//   k_text_starts<false>  one pass over the bytes, 16 per lane: byte p starts a line iff p = 0 or byte p - 1 is LF;
//                         line starts per 4 KiB tile
//   k_text_scan           exclusive scan of the tile counts (one workgroup); the record count M stays on the device
//   k_text_starts<true>   the same pass again with the tile (and the 80 bytes behind it) in LDS: a line start's record
//                         index is (tile offset) + (starts of the lanes before) + (starts before it in the lane); the lane
//                         that holds the start parses the line, reading forward into the next tile if it must.  A FAST line
//                         leaves as pos1 / pos2 / count; any other line leaves the outputs alone and is appended to the flag
//                         list as (record, byte offset, kind).
// This is the fused form: no array of line offsets exists, the text is read twice by cgcn_text_parse (12 bytes per tile of
// counts between the passes).  The scan is a copy of k_hic_scan's body (cgcn_hic.hip) because the two files are separate
// translation units; the Hi-C kernels are untouched.
// The value of a fast line is ONE correctly rounded fp64 operation on two exact operands (w < 10^15 < 2^53 times or divided
// by an exact power of ten <= 10^22): this file must not be compiled with fast-math or reciprocal division.
// Record indices and the flag order aside (the flag list is appended with an atomic counter; the wrapper sorts it), every
// write is a pure function of the text: two parses give the same bits.
#include "cgcn_common.hpp"

#define TEXT_THREADS 256
#define TEXT_CHUNK 16                                  // bytes per lane
#define TEXT_TILE (TEXT_THREADS * TEXT_CHUNK)          // bytes per workgroup
#define TEXT_LINE_MAX CGCN_TEXT_LINE_MAX               // bytes of a fast line, terminator excluded
#define TEXT_SCAN (TEXT_LINE_MAX + 2)                  // a line start looks this far for its LF: the line, CR, LF
#define TEXT_OVER 80                                   // bytes behind the tile kept in LDS (>= TEXT_SCAN - 1, a multiple of 16)

typedef unsigned long long u64;

__device__ const double TEXT_P10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                        1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
__device__ const u64 TEXT_P10U[16] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull, 100000000ull,
                                      1000000000ull, 10000000000ull, 100000000000ull, 1000000000000ull, 10000000000000ull,
                                      100000000000000ull, 1000000000000000ull};

// the 16 bytes at g (g a multiple of 16, g < n); bytes at or behind n read as 0.  The text base is 16-byte aligned.
__device__ __forceinline__ u32x4 text_load16(const unsigned char* __restrict__ text, long long n, long long g) {
  if (g + TEXT_CHUNK <= n) return *(const u32x4*)(text + g);
  u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < TEXT_CHUNK; ++k)
    if (g + k < n) v[k >> 2] |= (uint32_t)text[g + k] << ((k & 3) * 8);
  return v;
}

// bit k: byte g + k starts a line (it exists, and it is byte 0 or follows an LF)
__device__ __forceinline__ unsigned text_start_mask(const u32x4 v, bool after_lf, long long n, long long g) {
  unsigned lf = 0;
#pragma unroll
  for (int k = 0; k < TEXT_CHUNK; ++k) lf |= (((v[k >> 2] >> ((k & 3) * 8)) & 0xFFu) == 0x0Au ? 1u : 0u) << k;
  const unsigned starts = ((lf << 1) | (after_lf ? 1u : 0u)) & 0xFFFFu;
  const long long left = n - g;
  return left >= TEXT_CHUNK ? starts : (left <= 0 ? 0u : starts & ((1u << (int)left) - 1u));
}

// One line from its first byte s[0] (LDS); `to_eof` bytes lie between it and the end of the text.  Returns the kind:
// 0 fast (a, b, v are the record), CGCN_TEXT_SLOW, CGCN_TEXT_MALFORMED.  Reads s[0 .. min(to_eof, TEXT_SCAN)) only.
__device__ __forceinline__ int text_parse_line(const unsigned char* s, long long to_eof, int& a, int& b, double& v) {
  const int lim = to_eof < TEXT_SCAN ? (int)to_eof : TEXT_SCAN;
  int len = 0, tabs = 0;
  bool lf = false;
  for (; len < lim; ++len) {
    const unsigned c = s[len];
    if (c == 0x0Au) { lf = true; break; }
    tabs += c == 0x09u;
  }
  if (!lf && len < to_eof) return CGCN_TEXT_SLOW;      // no LF within the bound
  if (lf && len > 0 && s[len - 1] == 0x0Du) --len;     // CR LF
  if (len > TEXT_LINE_MAX) return CGCN_TEXT_SLOW;
  if (len == 0 || tabs != 2) return CGCN_TEXT_MALFORMED;
  int p = 0;
  int pos[2];
#pragma unroll
  for (int f = 0; f < 2; ++f) {   // one to ten digits, below 2^31, then the TAB
    u64 x = 0;
    int nd = 0;
    for (; p < len; ++p, ++nd) {
      const unsigned d = (unsigned)s[p] - 0x30u;
      if (d > 9u) break;
      x = x * 10ull + d;
    }
    if (nd < 1 || nd > 10 || x >= 2147483648ull || p >= len || s[p] != 0x09u) return CGCN_TEXT_SLOW;
    pos[f] = (int)x;
    ++p;
  }
  bool neg = false, eneg = false;
  if (p < len && (s[p] == 0x2Bu || s[p] == 0x2Du)) { neg = s[p] == 0x2Du; ++p; }
  u64 w = 0;           // the significand without leading zeros and trailing fractional zeros; never beyond 15 digits: no wrap
  int nsig = 0;        // its digits
  int nint = 0, nfr = 0, fr = 0, z = 0, ex = 0, nex = 0;   // fr: fractional digits inside w; z: fractional zeros not yet in w
  for (; p < len; ++p, ++nint) {
    const unsigned d = (unsigned)s[p] - 0x30u;
    if (d > 9u) break;
    if (nsig > 0 || d != 0u) {   // leading zeros do not count; beyond 15 digits the line is slow and w stays as it is
      ++nsig;
      if (nsig <= 15) w = w * 10ull + d;
    }
  }
  if (nint < 1) return CGCN_TEXT_SLOW;
  if (p < len && s[p] == 0x2Eu) {
    for (++p; p < len; ++p, ++nfr) {
      const unsigned d = (unsigned)s[p] - 0x30u;
      if (d > 9u) break;
      if (d == 0u) { ++z; continue; }
      if (nsig == 0) { w = d; nsig = 1; }
      else { nsig += z + 1; if (nsig <= 15) w = w * TEXT_P10U[z + 1] + d; }
      fr += z + 1;
      z = 0;
    }
    if (nfr < 1) return CGCN_TEXT_SLOW;
  }
  if (p < len && (s[p] | 0x20u) == 0x65u) {
    ++p;
    if (p < len && (s[p] == 0x2Bu || s[p] == 0x2Du)) { eneg = s[p] == 0x2Du; ++p; }
    for (; p < len; ++p, ++nex) {
      const unsigned d = (unsigned)s[p] - 0x30u;
      if (d > 9u) break;
      ex = ex < 10000 ? ex * 10 + (int)d : ex;
    }
    if (nex < 1) return CGCN_TEXT_SLOW;
  }
  const int e = (eneg ? -ex : ex) - fr;
  if (p != len || nsig > 15 || e > 22 || e < -22) return CGCN_TEXT_SLOW;
  const double m = (double)w;                          // exact: w < 10^15
  const double r = e >= 0 ? m * TEXT_P10[e] : m / TEXT_P10[-e];   // one rounding
  a = pos[0];
  b = pos[1];
  v = neg ? -r : r;
  return 0;
}

// sum of `c` over the lanes before this one (all 64 lanes active)
__device__ __forceinline__ int text_lanes_before(int c, int lane) {
  int inc = c;
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const int t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  return inc - c;
}

// PARSE = false: tile_counts[tile] = line starts in the tile.  PARSE = true: the records of the lines that start in the tile.
template <bool PARSE>
__global__ __launch_bounds__(TEXT_THREADS) void k_text_starts(const unsigned char* __restrict__ text, long long n,
                                                              int* __restrict__ tile_counts, const long long* __restrict__ tile_off,
                                                              long long M, int* __restrict__ pos1, int* __restrict__ pos2,
                                                              double* __restrict__ count, long long* __restrict__ flags,
                                                              long long flag_capacity, u64* __restrict__ flag_totals,
                                                              u64* __restrict__ flag_next) {
  __shared__ __attribute__((aligned(16))) unsigned char tile[PARSE ? TEXT_TILE + TEXT_OVER : 16];
  __shared__ int wave_tot[TEXT_THREADS / WAVE];
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  const long long base = (long long)blockIdx.x * TEXT_TILE;
  const long long g = base + (long long)threadIdx.x * TEXT_CHUNK;
  u32x4 v = {0u, 0u, 0u, 0u};
  bool after_lf = false;
  if (g < n) {
    v = text_load16(text, n, g);
    after_lf = g == 0 || text[g - 1] == 0x0Au;
  }
  const unsigned starts = text_start_mask(v, after_lf, n, g);
  const int mine = __popc(starts);
  const int before = text_lanes_before(mine, lane);
  if (lane == WAVE - 1) wave_tot[w] = before + mine;
  if (PARSE) {
    *(u32x4*)(tile + threadIdx.x * TEXT_CHUNK) = v;
    if (threadIdx.x < TEXT_OVER / TEXT_CHUNK) {
      const long long go = base + TEXT_TILE + (long long)threadIdx.x * TEXT_CHUNK;
      u32x4 o = {0u, 0u, 0u, 0u};
      if (go < n) o = text_load16(text, n, go);
      *(u32x4*)(tile + TEXT_TILE + threadIdx.x * TEXT_CHUNK) = o;
    }
  }
  __syncthreads();
  if (!PARSE) {
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
    return;
  }
  long long r = tile_off[blockIdx.x] + before;
  for (int k = 0; k < w; ++k) r += wave_tot[k];
  for (unsigned m = starts; m; m &= m - 1u, ++r) {
    const int rel = threadIdx.x * TEXT_CHUNK + (__ffs(m) - 1);   // rel + TEXT_SCAN <= TEXT_TILE + TEXT_OVER
    if (r >= M) break;                                           // the caller's M is below the record count: nothing is overrun
    int a = 0, b = 0;
    double val = 0.0;
    const int kind = text_parse_line(tile + rel, n - (base + rel), a, b, val);
    if (kind == 0) {
      pos1[r] = a;
      pos2[r] = b;
      count[r] = val;
    } else {
      atomicAdd(&flag_totals[kind - 1], 1ull);
      const u64 slot = atomicAdd(flag_next, 1ull);
      if (slot < (u64)flag_capacity) {
        flags[3 * slot] = r;
        flags[3 * slot + 1] = base + rel;
        flags[3 * slot + 2] = kind;
      }
    }
  }
}

// exclusive scan of counts[0..nb) into off[0..nb); the total goes to total[0].  One workgroup of 1024 threads.
__global__ __launch_bounds__(1024) void k_text_scan(int nb, const int* __restrict__ counts, long long* __restrict__ off,
                                                    long long* __restrict__ total) {
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
  if (t == 1023) total[0] = part[1023];
}

struct TextPlan {
  long long tiles;
  size_t o_counts, o_off, o_total, o_next, total;
};

static inline size_t text_al(size_t x) { return (x + 255) & ~(size_t)255; }

static bool text_plan(long long n_bytes, TextPlan* p) {
  if (n_bytes < 0) return false;
  p->tiles = (n_bytes + TEXT_TILE - 1) / TEXT_TILE;
  if (p->tiles < 1) p->tiles = 1;
  if (p->tiles >= 2147483647ll) return false;
  size_t o = 0;
  p->o_counts = o; o += text_al((size_t)p->tiles * 4);
  p->o_off = o; o += text_al((size_t)p->tiles * 8);
  p->o_total = o; o += 256;
  p->o_next = o; o += 256;
  p->total = o + 256;   // the base is rounded up to 256 bytes
  return true;
}

// tile counts and offsets of the text; the record count goes to n_records
static void text_count(hipStream_t st, const TextPlan& p, char* w, const unsigned char* text, long long n, long long* n_records) {
  hipLaunchKernelGGL(k_text_starts<false>, dim3((unsigned)p.tiles), dim3(TEXT_THREADS), 0, st, text, n, (int*)(w + p.o_counts),
                     (const long long*)nullptr, 0ll, (int*)nullptr, (int*)nullptr, (double*)nullptr, (long long*)nullptr, 0ll,
                     (u64*)nullptr, (u64*)nullptr);
  hipLaunchKernelGGL(k_text_scan, dim3(1), dim3(1024), 0, st, (int)p.tiles, (const int*)(w + p.o_counts), (long long*)(w + p.o_off),
                     n_records);
}

extern "C" {

size_t cgcn_text_workspace_bytes(long long n_bytes) {
  TextPlan p;
  return text_plan(n_bytes, &p) ? p.total : 0;
}

int cgcn_text_count(cgcn_stream_t stream, const void* text, long long n_bytes, void* workspace, size_t workspace_bytes,
                    long long* n_records) {
  if (n_bytes < 0 || !n_records) return CGCN_ERR_BAD_ARG;
  if (n_bytes > 0 && (!text || !workspace || misaligned16(text))) return CGCN_ERR_BAD_ARG;
  TextPlan p;
  if (!text_plan(n_bytes, &p)) return CGCN_ERR_UNSUPPORTED;
  if (n_bytes > 0 && workspace_bytes < p.total) return CGCN_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (n_bytes == 0) return hipMemsetAsync(n_records, 0, 8, st) == hipSuccess ? CGCN_OK : CGCN_ERR_LAUNCH;
  char* w = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  text_count(st, p, w, (const unsigned char*)text, n_bytes, n_records);
  return launch_status();
}

int cgcn_text_parse(cgcn_stream_t stream, const void* text, long long n_bytes, long long M, int32_t* pos1_out, int32_t* pos2_out,
                    double* count_out, long long* flags, long long flag_capacity, long long* flag_totals, void* workspace,
                    size_t workspace_bytes) {
  if (n_bytes < 0 || M < 0 || flag_capacity < 0 || !flag_totals) return CGCN_ERR_BAD_ARG;
  if (n_bytes > 0 && (!text || !workspace || misaligned16(text))) return CGCN_ERR_BAD_ARG;
  if (M > 0 && (!pos1_out || !pos2_out || !count_out)) return CGCN_ERR_BAD_ARG;
  if (flag_capacity > 0 && !flags) return CGCN_ERR_BAD_ARG;
  if (M >= 2147483648ll) return CGCN_ERR_UNSUPPORTED;
  TextPlan p;
  if (!text_plan(n_bytes, &p)) return CGCN_ERR_UNSUPPORTED;
  if (n_bytes > 0 && workspace_bytes < p.total) return CGCN_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(flag_totals, 0, 16, st) != hipSuccess) return CGCN_ERR_LAUNCH;
  if (n_bytes == 0 || M == 0) return CGCN_OK;
  char* w = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  if (hipMemsetAsync(w + p.o_next, 0, 8, st) != hipSuccess) return CGCN_ERR_LAUNCH;
  text_count(st, p, w, (const unsigned char*)text, n_bytes, (long long*)(w + p.o_total));
  hipLaunchKernelGGL(k_text_starts<true>, dim3((unsigned)p.tiles), dim3(TEXT_THREADS), 0, st, (const unsigned char*)text, n_bytes,
                     (int*)nullptr, (const long long*)(w + p.o_off), M, pos1_out, pos2_out, count_out, flags, flag_capacity,
                     (u64*)flag_totals, (u64*)(w + p.o_next));
  return launch_status();
}

}  // extern "C"
