// chromegcn_amd/csrc/cgcn_text.hip
//
// Hi-C contact text (`RAWobserved`: pos1<TAB>pos2<TAB>count per line) parsed on the device into the arrays HicContacts holds
// (the rule is stated once in include/chromegcn.h above cgcn_text_count).
//
//   k_text_starts<false>  one pass over the bytes, 16 per lane: byte p starts a line iff p = 0 or byte p - 1 is LF;
//                         line starts per 4 KiB tile
//   k_tile_scan           exclusive scan of the tile counts (one workgroup); the record count M stays on the device
//   k_text_starts<true>   the same pass again with the tile (and the 80 bytes behind it) in LDS: a line start's record
//                         index is (tile offset) + (starts of the lanes before) + (starts before it in the lane); the lane
//                         that holds the start parses the line, reading forward into the next tile if it must.  A FAST line
//                         leaves as pos1 / pos2 / count; any other line leaves the outputs alone and is appended to the flag
//                         list as (record, byte offset, kind).
// This is the fused form: no array of line offsets exists, the text is read twice by cgcn_text_parse (12 bytes per tile of
// counts between the passes).  The scan, the line-start front end and the workspace helpers are cgcn_compact.hpp's.
// The value of a fast line is ONE correctly rounded fp64 operation on two exact operands (w < 10^15 < 2^53 times or divided
// by an exact power of ten <= 10^22): this file must not be compiled with fast-math or reciprocal division.
// Record indices and the flag order aside (the flag list is appended with an atomic counter; the wrapper sorts it), every
// write is a pure function of the text: two parses give the same bits.
#include "cgcn_compact.hpp"

#define TEXT_THREADS LINES_THREADS
#define TEXT_CHUNK LINES_CHUNK                         // bytes per lane
#define TEXT_TILE LINES_TILE                           // bytes per workgroup
#define TEXT_LINE_MAX CGCN_TEXT_LINE_MAX               // bytes of a fast line, terminator excluded
#define TEXT_SCAN (TEXT_LINE_MAX + 2)                  // a line start looks this far for its LF: the line, CR, LF
#define TEXT_OVER 80                                   // bytes behind the tile kept in LDS (>= TEXT_SCAN - 1, a multiple of 16)

__device__ const double TEXT_P10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                        1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
__device__ const u64 TEXT_P10U[16] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull, 100000000ull,
                                      1000000000ull, 10000000000ull, 100000000000ull, 1000000000000ull, 10000000000000ull,
                                      100000000000000ull, 1000000000000000ull};

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
  const long long base = (long long)blockIdx.x * TEXT_TILE;
  const LinesFront f = lines_tile_front(text, n, wave_tot);
  if (PARSE) {
    *(u32x4*)(tile + threadIdx.x * TEXT_CHUNK) = f.v;
    if (threadIdx.x < TEXT_OVER / TEXT_CHUNK) {
      const long long go = base + TEXT_TILE + (long long)threadIdx.x * TEXT_CHUNK;
      u32x4 o = {0u, 0u, 0u, 0u};
      if (go < n) o = lines_load16(text, n, go);
      *(u32x4*)(tile + TEXT_TILE + threadIdx.x * TEXT_CHUNK) = o;
    }
  }
  __syncthreads();
  if (!PARSE) {
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = wg_count(wave_tot);
    return;
  }
  long long r = wg_before(tile_off[blockIdx.x] + f.before, wave_tot);
  for (unsigned m = f.starts; m; m &= m - 1u, ++r) {
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

struct TextPlan {
  long long tiles;
  size_t o_counts, o_off, o_total, o_next, total;
};

static bool text_plan(long long n_bytes, TextPlan* p) {
  if (n_bytes < 0) return false;
  p->tiles = tiles_of(n_bytes, TEXT_TILE);
  if (p->tiles >= 2147483647ll) return false;
  WsBump b = {0};
  p->o_counts = b.take((size_t)p->tiles * 4);
  p->o_off = b.take((size_t)p->tiles * 8);
  p->o_total = b.take(256);
  p->o_next = b.take(256);
  p->total = b.o + 256;   // the base is rounded up to 256 bytes
  return true;
}

// tile counts and offsets of the text; the record count goes to n_records
static void text_count(hipStream_t st, const TextPlan& p, char* w, const unsigned char* text, long long n, long long* n_records) {
  hipLaunchKernelGGL(k_text_starts<false>, dim3((unsigned)p.tiles), dim3(TEXT_THREADS), 0, st, text, n, (int*)(w + p.o_counts),
                     (const long long*)nullptr, 0ll, (int*)nullptr, (int*)nullptr, (double*)nullptr, (long long*)nullptr, 0ll,
                     (u64*)nullptr, (u64*)nullptr);
  hipLaunchKernelGGL(k_tile_scan<>, dim3(1), dim3(1024), 0, st, (int)p.tiles, (const int*)(w + p.o_counts), (long long*)(w + p.o_off),
                     n_records, (int*)nullptr, 0ll);
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
  char* w = ws_base(workspace);
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
  char* w = ws_base(workspace);
  if (hipMemsetAsync(w + p.o_next, 0, 8, st) != hipSuccess) return CGCN_ERR_LAUNCH;
  text_count(st, p, w, (const unsigned char*)text, n_bytes, (long long*)(w + p.o_total));
  hipLaunchKernelGGL(k_text_starts<true>, dim3((unsigned)p.tiles), dim3(TEXT_THREADS), 0, st, (const unsigned char*)text, n_bytes,
                     (int*)nullptr, (const long long*)(w + p.o_off), M, pos1_out, pos2_out, count_out, flags, flag_capacity,
                     (u64*)flag_totals, (u64*)(w + p.o_next));
  return launch_status();
}

}  // extern "C"
