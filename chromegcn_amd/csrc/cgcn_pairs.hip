// chromegcn_amd/csrc/cgcn_pairs.hip
//
// Read-pair text (HiC-Pro `allValidPairs`: one line per pair, TAB-separated, twelve or thirteen columns) turned into the contact
// records HicContacts holds (the rule is stated once in include/chromegcn.h above
// cgcn_pairs_parse_workspace_bytes).  The text arrives in chunks of whole lines; the kept pairs stay on the device as 64-bit keys.
//
// cgcn_pairs_parse, one chunk:
//   k_pairs_starts<false>  one pass over the bytes, 16 per lane: line starts per 4 KiB tile (as k_text_starts of cgcn_text.hip)
//   k_tile_scan            exclusive scan of the tile counts (one workgroup): the line number of every tile's first line
//   k_pairs_starts<true>   the tile and the 272 bytes behind it in LDS with the table of chromosome names; the line starts of the
//                          tile are listed in LDS in order and handed out to consecutive lanes, so that the lanes that walk lines
//                          sit in as few waves as the tile allows.  The lane that owns a line start walks its line (the line is
//                          parsed once, by the tile it starts in, reading forward into the next tile if it must): finds the TABs
//                          of the first six fields, compares field 2 with field 5 and with the name table, parses the two
//                          integers, bins them, applies min_diff.  A kept pair's key goes to the tile's slot of a temporary at
//                          its rank among the tile's kept pairs; a line that is not FAST goes to the flag list as (line, byte
//                          offset, kind, rank among the kept pairs in front of it).
//   k_tile_scan            exclusive scan of the kept counts per tile
//   k_pairs_compact        the tiles' keys, in order, behind the keys of the earlier chunks: keys[kept so far + ...]
//   k_pairs_finish         ranks of the flag list made global; the chunk's class totals added to the running totals
// The running totals (device int64 [8]) are read once at the start of a call (copied into the workspace: the line number and
// the key index this chunk starts at) and written once at its end; nothing else is kept between calls.
//
// cgcn_pairs_reduce, once: rocprim::radix_sort_keys over bits 1..62 of the keys (the swap bit is not sorted on),
//   k_pairs_heads<false> / k_tile_scan / k_pairs_heads<true> (a key starts a record iff it differs from the one before above
//   bit 0; the record's positions, its first key and the chromosome offsets), k_pairs_counts (count = distance to the next
//   record's first key, as fp64).
//
// Integer arithmetic only: pos / resolution is a multiply-high by floor(2^64 / res) + 1, exact for pos < 2^31 (the error term
// pos / 2^64 < 2^-33 is below 1 / res), so not even the compiler's division sequence (which goes through v_rcp_f32) is used.
// The one conversion is the count's int -> fp64 in k_pairs_counts.  Flag order aside (an atomic counter; the wrapper sorts),
// every write is a pure function of the text and the parameters: two runs give the same bits.
#include <cstring>  // rocprim 4.x headers use memset without including it
#include <rocprim/rocprim.hpp>

#include "cgcn_compact.hpp"

#define PAIRS_THREADS LINES_THREADS
#define PAIRS_CHUNK LINES_CHUNK                          // bytes per lane
#define PAIRS_TILE LINES_TILE                            // bytes per workgroup
#define PAIRS_LINE_MAX CGCN_PAIRS_LINE_MAX               // bytes of a fast line, terminator excluded
#define PAIRS_SCAN (PAIRS_LINE_MAX + 2)                  // a line start looks this far for its LF: the line, CR, LF
#define PAIRS_OVER 272                                   // bytes behind the tile kept in LDS (>= PAIRS_SCAN - 1, a multiple of 16)
// kept pairs per tile: a kept line is at least `TAB c TAB 1 TAB TAB c TAB 2 LF` = 10 bytes, so at most 410 start in 4096 bytes
#define PAIRS_TILE_KEYS 416
#define PAIRS_NAMES CGCN_PAIRS_MAX_CHROMS
#define RED_THREADS 256
#define RED_ITEMS 4
#define RED_TILE (RED_THREADS * RED_ITEMS)

// the class of a line: its index in the totals
enum { LINE_EMPTY = CGCN_PAIRS_T_EMPTY, LINE_KEPT = CGCN_PAIRS_T_KEPT, LINE_INTER = CGCN_PAIRS_T_INTER_CHROM,
       LINE_OTHER = CGCN_PAIRS_T_OTHER_CHROM, LINE_CLOSE = CGCN_PAIRS_T_TOO_CLOSE, LINE_SLOW = CGCN_PAIRS_T_SLOW,
       LINE_MALFORMED = CGCN_PAIRS_T_MALFORMED };

struct PairsRule {
  int n_chroms, binning;
  unsigned res;
  u64 magic;            // floor(2^64 / res) + 1
  long long min_diff;
};

// a name of 1 to 15 bytes between s[p] and the TAB behind it, packed: bytes 0-7 in lo, 8-14 in hi, the length in hi's top
// byte.  Returns the length (which may exceed 15: the packed form then means nothing); p is left on the TAB.
__device__ __forceinline__ int pairs_name(const unsigned char* s, int& p, u64& lo, u64& hi) {
  int len = 0;
  lo = hi = 0;
  for (;; ++p, ++len) {
    const u64 c = s[p];
    if (c == 0x09ull) break;
    const u64 v = c << (8 * (len & 7));                   // selects, not branches: no indexed pair in scratch
    lo |= len < 8 ? v : 0ull;
    hi |= len >= 8 && len < 15 ? v : 0ull;
  }
  hi |= (u64)(len & 0xFF) << 56;
  return len;
}

// one to ten decimal digits between s[p] and the TAB or the line's end behind them, below 2^31: true, and x is the value
__device__ __forceinline__ bool pairs_digits(const unsigned char* s, int& p, int len, u64& x) {
  int nd = 0;
  bool ok = true;
  x = 0;
  for (; p < len; ++p, ++nd) {
    const unsigned c = s[p];
    if (c == 0x09u) break;
    const unsigned d = c - 0x30u;
    ok = ok && d <= 9u && nd < 10;
    x = nd < 10 ? x * 10ull + (d & 15u) : x;
  }
  return ok && nd >= 1 && x < 2147483648ull;
}

// the bin of x < 2^31 (its position divided by res); false when the binned position is 2^31 or more
__device__ __forceinline__ bool pairs_bin(u64 x, const PairsRule& R, u64& bin) {
  const u64 q = __umul64hi(x, R.magic);
  const u64 r = x - q * R.res;
  u64 b = q;
  if (R.binning == CGCN_PAIRS_NEAREST) b += (2ull * r > R.res || (2ull * r == R.res && (q & 1ull))) ? 1ull : 0ull;
  bin = b;
  return b * R.res < 2147483648ull;
}

// One line from its first byte s[0] (LDS); `to_eof` bytes lie between it and the end of the text.  Returns the LINE_* class;
// key is the pair's key when it is LINE_KEPT.  Reads s[0 .. min(to_eof, PAIRS_SCAN)) only.
__device__ __forceinline__ int pairs_parse_line(const unsigned char* s, long long to_eof, const PairsRule& R, const u64* names,
                                                u64& key) {
  const int lim = to_eof < PAIRS_SCAN ? (int)to_eof : PAIRS_SCAN;
  int len = 0, tabs = 0;
  bool lf = false, bad = false, cr = false;   // bad: a `"` byte or a CR that no LF follows; cr: the byte before was a CR
  for (; len < lim; ++len) {
    const unsigned c = s[len];
    if (c == 0x0Au) { lf = true; break; }
    bad = bad || cr || c == 0x22u;
    cr = c == 0x0Du;
    tabs += c == 0x09u;
  }
  if (!lf && len < to_eof) return LINE_SLOW;             // no LF within the bound
  if (lf && cr) --len;                                   // CR LF
  else bad = bad || cr;                                  // a CR that ends the text
  if (len > PAIRS_LINE_MAX) return LINE_SLOW;
  if (len == 0 && !bad) return LINE_EMPTY;
  if (bad || tabs < 5) return LINE_MALFORMED;
  int p = 0;
  while (s[p] != 0x09u) ++p;                             // field 1; five TABs lie inside the line
  ++p;
  u64 alo, ahi, blo, bhi, x1, x2;
  const int la = pairs_name(s, p, alo, ahi);
  ++p;
  const bool d1 = pairs_digits(s, p, len, x1);
  ++p;
  while (s[p] != 0x09u) ++p;                             // field 4
  ++p;
  const int lb = pairs_name(s, p, blo, bhi);
  ++p;
  const bool d2 = pairs_digits(s, p, len, x2);
  if (la < 1 || la > CGCN_PAIRS_NAME_MAX || lb < 1 || lb > CGCN_PAIRS_NAME_MAX || !d1 || !d2) return LINE_SLOW;
  if (alo != blo || ahi != bhi) return LINE_INTER;
  u64 b1, b2;
  if (!pairs_bin(x1, R, b1) || !pairs_bin(x2, R, b2)) return LINE_MALFORMED;
  int idx = -1;
  for (int c = 0; c < R.n_chroms; ++c)
    if (names[2 * c] == alo && names[2 * c + 1] == ahi) idx = c;
  if (idx < 0) return LINE_OTHER;
  const u64 lo = b1 < b2 ? b1 : b2, hi = b1 < b2 ? b2 : b1;
  if ((long long)((hi - lo) * R.res) <= R.min_diff) return LINE_CLOSE;
  key = ((u64)idx << 57) | (lo << 29) | (hi << 1) | (b1 > b2 ? 1ull : 0ull);
  return LINE_KEPT;
}

// workspace scalars (int64 words)
enum { WS_LINES = 0, WS_KEPT, WS_FLAG_NEXT, WS_BASE = 8, WS_CLASS = 16, WS_WORDS = 32 };

// PARSE = false: tile_counts[tile] = line starts in the tile.  PARSE = true: the pairs of the lines that start in the tile.
template <bool PARSE>
__global__ __launch_bounds__(PAIRS_THREADS) void k_pairs_starts(const unsigned char* __restrict__ text, long long n,
                                                                int* __restrict__ tile_counts, const long long* __restrict__ tile_off,
                                                                PairsRule R, const u64* __restrict__ names_g, long long byte_base,
                                                                u64* __restrict__ tmp_keys, int* __restrict__ kept_counts,
                                                                long long* __restrict__ flags, long long flag_capacity,
                                                                u64* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) unsigned char tile[PARSE ? PAIRS_TILE + PAIRS_OVER : 16];
  __shared__ unsigned short lstart[PARSE ? PAIRS_TILE : 1];
  __shared__ u64 names[PARSE ? 2 * PAIRS_NAMES : 1];
  __shared__ int wave_tot[PAIRS_THREADS / WAVE];
  __shared__ unsigned cls[8];
  const long long base = (long long)blockIdx.x * PAIRS_TILE;
  const LinesFront f = lines_tile_front(text, n, wave_tot);
  if (PARSE) {
    *(u32x4*)(tile + threadIdx.x * PAIRS_CHUNK) = f.v;
    if (threadIdx.x < PAIRS_OVER / PAIRS_CHUNK) {
      const long long go = base + PAIRS_TILE + (long long)threadIdx.x * PAIRS_CHUNK;
      u32x4 o = {0u, 0u, 0u, 0u};
      if (go < n) o = lines_load16(text, n, go);
      *(u32x4*)(tile + PAIRS_TILE + threadIdx.x * PAIRS_CHUNK) = o;
    }
    if (threadIdx.x < 2 * R.n_chroms) names[threadIdx.x] = names_g[threadIdx.x];
    if (threadIdx.x < 8) cls[threadIdx.x] = 0u;
  }
  __syncthreads();
  if (!PARSE) {
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = wg_count(wave_tot);
    return;
  }
  int first = wg_before(f.before, wave_tot);
  const int n_lines = wg_count(wave_tot);
  for (unsigned m = f.starts; m; m &= m - 1u, ++first) lstart[first] = (unsigned short)(threadIdx.x * PAIRS_CHUNK + (__ffs(m) - 1));
  __syncthreads();                                       // wave_tot is reused below
  const long long line0 = (long long)ws[WS_BASE + CGCN_PAIRS_T_LINES] + tile_off[blockIdx.x];
  int kept_base = 0;                                     // kept pairs of the rounds before
  for (int i0 = 0; i0 < n_lines; i0 += PAIRS_THREADS) {  // n_lines is the same in every lane
    const int i = i0 + threadIdx.x;
    int kind = 0, rel = 0;
    u64 key = 0;
    if (i < n_lines) {
      rel = lstart[i];                                   // rel + PAIRS_SCAN <= PAIRS_TILE + PAIRS_OVER
      kind = pairs_parse_line(tile + rel, n - (base + rel), R, names, key);
      atomicAdd(&cls[kind], 1u);
    }
    const WgFlags<> kept(kind == LINE_KEPT, wave_tot);
    const int rank = kept.before(kept_base);
    kept_base += kept.count();
    if (kind == LINE_KEPT) {
      if (rank < PAIRS_TILE_KEYS) tmp_keys[(size_t)blockIdx.x * PAIRS_TILE_KEYS + rank] = key;
    } else if (kind == LINE_SLOW || kind == LINE_MALFORMED) {
      const u64 slot = atomicAdd(&ws[WS_FLAG_NEXT], 1ull);
      if (slot < (u64)flag_capacity) {
        flags[4 * slot] = line0 + i;
        flags[4 * slot + 1] = byte_base + base + rel;
        flags[4 * slot + 2] = kind == LINE_SLOW ? CGCN_PAIRS_SLOW : CGCN_PAIRS_MALFORMED;
        flags[4 * slot + 3] = rank;                      // within the tile; k_pairs_finish makes it global
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) kept_counts[blockIdx.x] = kept_base < PAIRS_TILE_KEYS ? kept_base : PAIRS_TILE_KEYS;
  if (threadIdx.x >= 1 && threadIdx.x < 8 && threadIdx.x != LINE_KEPT && cls[threadIdx.x]) atomicAdd(&ws[WS_CLASS + threadIdx.x], (u64)cls[threadIdx.x]);
}

// the keys of tile blockIdx.x behind the keys of the tiles and the chunks before it
__global__ __launch_bounds__(PAIRS_THREADS) void k_pairs_compact(const u64* __restrict__ tmp_keys, const int* __restrict__ kept_counts,
                                                                 const long long* __restrict__ kept_off, const u64* __restrict__ ws,
                                                                 u64* __restrict__ keys, long long key_capacity) {
  const int cnt = kept_counts[blockIdx.x];
  const long long dst = (long long)ws[WS_BASE + CGCN_PAIRS_T_KEPT] + kept_off[blockIdx.x];
  for (int i = threadIdx.x; i < cnt; i += PAIRS_THREADS)
    if (dst + i < key_capacity) keys[dst + i] = tmp_keys[(size_t)blockIdx.x * PAIRS_TILE_KEYS + i];
}

// one workgroup: the flag list's ranks made global, the chunk's totals written and added to the running ones
__global__ __launch_bounds__(PAIRS_THREADS) void k_pairs_finish(long long* __restrict__ flags, long long flag_capacity,
                                                                long long byte_base, const long long* __restrict__ kept_off,
                                                                const u64* __restrict__ ws, long long* __restrict__ totals,
                                                                long long* __restrict__ chunk_totals) {
  const long long kept0 = (long long)ws[WS_BASE + CGCN_PAIRS_T_KEPT];
  const long long nf = (long long)ws[WS_FLAG_NEXT] < flag_capacity ? (long long)ws[WS_FLAG_NEXT] : flag_capacity;
  for (long long s = threadIdx.x; s < nf; s += PAIRS_THREADS)
    flags[4 * s + 3] += kept0 + kept_off[(flags[4 * s + 1] - byte_base) / PAIRS_TILE];
  if (threadIdx.x < 8) {
    const int k = threadIdx.x;
    const long long c = k == CGCN_PAIRS_T_LINES ? (long long)ws[WS_LINES] : k == CGCN_PAIRS_T_KEPT ? (long long)ws[WS_KEPT]
                                                                                                : (long long)ws[WS_CLASS + k];
    chunk_totals[k] = c;
    totals[k] = (long long)ws[WS_BASE + k] + c;
  }
}

// A key starts a record iff it is the first or differs from the key before above the swap bit.  WRITE = false: records per
// tile.  WRITE = true: the record's positions, its first key's index, and the chromosome offsets.
template <bool WRITE>
__global__ __launch_bounds__(RED_THREADS) void k_pairs_heads(long long n, const u64* __restrict__ keys, int* __restrict__ tile_counts,
                                                             const long long* __restrict__ tile_off,
                                                             const long long* __restrict__ n_records, int n_chroms, unsigned res,
                                                             int* __restrict__ pos1, int* __restrict__ pos2,
                                                             unsigned* __restrict__ first, long long* __restrict__ chrom_off) {
  __shared__ int wave_tot[RED_THREADS / WAVE];
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  const long long i0 = ((long long)blockIdx.x * RED_THREADS + threadIdx.x) * RED_ITEMS;
  u64 k[RED_ITEMS + 1];
  k[0] = i0 > 0 && i0 - 1 < n ? keys[i0 - 1] : 0ull;
  unsigned heads = 0;
#pragma unroll
  for (int j = 0; j < RED_ITEMS; ++j) {
    k[j + 1] = i0 + j < n ? keys[i0 + j] : 0ull;
    if (i0 + j < n && (i0 + j == 0 || (k[j + 1] >> 1) != (k[j] >> 1))) heads |= 1u << j;
  }
  const int mine = __popc(heads);
  const int before = wave_excl_sum(mine, lane);
  if (lane == WAVE - 1) wave_tot[w] = before + mine;
  __syncthreads();
  if (!WRITE) {
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = wg_count(wave_tot);
    return;
  }
  long long r = wg_before(tile_off[blockIdx.x] + before, wave_tot);
#pragma unroll
  for (int j = 0; j < RED_ITEMS; ++j) {
    if (i0 + j >= n) break;
    const int c = min((int)(k[j + 1] >> 57), n_chroms - 1);
    if (heads & (1u << j)) {
      pos1[r] = (int)(((k[j + 1] >> 29) & 0xFFFFFFFull) * res);
      pos2[r] = (int)(((k[j + 1] >> 1) & 0xFFFFFFFull) * res);
      first[r] = (unsigned)(i0 + j);
      const int cp = i0 + j == 0 ? -1 : min((int)(k[j] >> 57), n_chroms - 1);
      for (int q = cp + 1; q <= c; ++q) chrom_off[q] = r;   // every chromosome up to this one starts here
      ++r;
    }
    if (i0 + j == n - 1)
      for (int q = c + 1; q <= n_chroms; ++q) chrom_off[q] = n_records[0];
  }
}

__global__ __launch_bounds__(RED_THREADS) void k_pairs_counts(long long n, const long long* __restrict__ n_records,
                                                              const unsigned* __restrict__ first, double* __restrict__ count) {
  const long long r = (long long)blockIdx.x * RED_THREADS + threadIdx.x;
  const long long R = n_records[0];
  if (r >= R) return;
  const long long end = r + 1 < R ? (long long)first[r + 1] : n;
  count[r] = (double)(end - (long long)first[r]);
}

struct PairsPlan {
  long long tiles;
  size_t o_counts, o_off, o_kcounts, o_koff, o_ws, o_tmp, total;
};

static bool pairs_plan(long long n_bytes, PairsPlan* p) {
  if (n_bytes < 0) return false;
  p->tiles = tiles_of(n_bytes, PAIRS_TILE);
  if (p->tiles >= 2147483647ll) return false;
  WsBump b = {0};
  p->o_counts = b.take((size_t)p->tiles * 4);
  p->o_off = b.take((size_t)p->tiles * 8);
  p->o_kcounts = b.take((size_t)p->tiles * 4);
  p->o_koff = b.take((size_t)p->tiles * 8);
  p->o_ws = b.take(WS_WORDS * 8);
  p->o_tmp = b.take((size_t)p->tiles * PAIRS_TILE_KEYS * 8);
  p->total = b.o + 256;   // the base is rounded up to 256 bytes
  return true;
}

struct ReducePlan {
  long long tiles;
  size_t temp, o_sorted, o_first, o_counts, o_off, o_temp, total;
};

static bool reduce_plan(long long n_keys, ReducePlan* p) {
  if (n_keys < 0 || n_keys >= 2147483647ll) return false;
  const long long n = n_keys < 1 ? 1 : n_keys;
  p->tiles = tiles_of(n, RED_TILE);
  size_t t = 0;
  (void)rocprim::radix_sort_keys(nullptr, t, (const u64*)nullptr, (u64*)nullptr, (size_t)n, 1u, 63u);
  p->temp = t;
  WsBump b = {0};
  p->o_sorted = b.take((size_t)n * 8);
  p->o_first = b.take((size_t)n * 4);
  p->o_counts = b.take((size_t)p->tiles * 4);
  p->o_off = b.take((size_t)p->tiles * 8);
  p->o_temp = b.take(t);
  p->total = b.o + 256;
  return true;
}

extern "C" {

size_t cgcn_pairs_parse_workspace_bytes(long long n_bytes) {
  PairsPlan p;
  return pairs_plan(n_bytes, &p) ? p.total : 0;
}

int cgcn_pairs_parse(cgcn_stream_t stream, const void* text, long long n_bytes, long long byte_base, const void* names, int n_chroms,
                     int resolution_bp, int binning, long long min_diff, unsigned long long* keys, long long key_capacity,
                     long long* flags, long long flag_capacity, long long* totals, long long* chunk_totals, void* workspace,
                     size_t workspace_bytes) {
  if (n_bytes < 0 || byte_base < 0 || key_capacity < 0 || flag_capacity < 0 || !totals || !chunk_totals || !names || !workspace)
    return CGCN_ERR_BAD_ARG;
  if (n_bytes > 0 && (!text || misaligned16(text))) return CGCN_ERR_BAD_ARG;
  if ((key_capacity > 0 && !keys) || (flag_capacity > 0 && !flags) || ((uintptr_t)names & 7u)) return CGCN_ERR_BAD_ARG;
  if (binning != CGCN_PAIRS_NEAREST && binning != CGCN_PAIRS_FLOOR) return CGCN_ERR_BAD_ARG;
  if (n_chroms < 1 || n_chroms > CGCN_PAIRS_MAX_CHROMS || resolution_bp < 8) return CGCN_ERR_UNSUPPORTED;
  PairsPlan p;
  if (!pairs_plan(n_bytes, &p)) return CGCN_ERR_UNSUPPORTED;
  if (workspace_bytes < p.total) return CGCN_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* w = ws_base(workspace);
  u64* ws = (u64*)(w + p.o_ws);
  if (hipMemsetAsync(ws, 0, WS_WORDS * 8, st) != hipSuccess) return CGCN_ERR_LAUNCH;
  if (hipMemcpyAsync(ws + WS_BASE, totals, 64, hipMemcpyDeviceToDevice, st) != hipSuccess) return CGCN_ERR_LAUNCH;
  PairsRule R;
  R.n_chroms = n_chroms;
  R.binning = binning;
  R.res = (unsigned)resolution_bp;
  R.magic = ~0ull / (u64)resolution_bp + 1ull;
  R.min_diff = min_diff;
  if (n_bytes > 0) {
    const unsigned char* t = (const unsigned char*)text;
    hipLaunchKernelGGL(k_pairs_starts<false>, dim3((unsigned)p.tiles), dim3(PAIRS_THREADS), 0, st, t, n_bytes, (int*)(w + p.o_counts),
                       (const long long*)nullptr, R, (const u64*)nullptr, 0ll, (u64*)nullptr, (int*)nullptr, (long long*)nullptr, 0ll,
                       (u64*)nullptr);
    hipLaunchKernelGGL(k_tile_scan<>, dim3(1), dim3(1024), 0, st, (int)p.tiles, (const int*)(w + p.o_counts), (long long*)(w + p.o_off),
                       (long long*)(ws + WS_LINES), (int*)nullptr, 0ll);
    hipLaunchKernelGGL(k_pairs_starts<true>, dim3((unsigned)p.tiles), dim3(PAIRS_THREADS), 0, st, t, n_bytes, (int*)nullptr,
                       (const long long*)(w + p.o_off), R, (const u64*)names, byte_base, (u64*)(w + p.o_tmp), (int*)(w + p.o_kcounts),
                       flags, flag_capacity, ws);
    hipLaunchKernelGGL(k_tile_scan<>, dim3(1), dim3(1024), 0, st, (int)p.tiles, (const int*)(w + p.o_kcounts),
                       (long long*)(w + p.o_koff), (long long*)(ws + WS_KEPT), (int*)nullptr, 0ll);
    hipLaunchKernelGGL(k_pairs_compact, dim3((unsigned)p.tiles), dim3(PAIRS_THREADS), 0, st, (const u64*)(w + p.o_tmp),
                       (const int*)(w + p.o_kcounts), (const long long*)(w + p.o_koff), (const u64*)ws, (u64*)keys, key_capacity);
  }
  hipLaunchKernelGGL(k_pairs_finish, dim3(1), dim3(PAIRS_THREADS), 0, st, flags, flag_capacity, byte_base,
                     (const long long*)(w + p.o_koff), (const u64*)ws, totals, chunk_totals);
  return launch_status();
}

size_t cgcn_pairs_reduce_workspace_bytes(long long n_keys) {
  ReducePlan p;
  return reduce_plan(n_keys, &p) ? p.total : 0;
}

int cgcn_pairs_reduce(cgcn_stream_t stream, long long n_keys, const unsigned long long* keys, int n_chroms, int resolution_bp,
                      int32_t* pos1_out, int32_t* pos2_out, double* count_out, long long* chrom_offsets, long long* n_records,
                      void* workspace, size_t workspace_bytes) {
  if (n_keys < 0 || !chrom_offsets || !n_records || !workspace) return CGCN_ERR_BAD_ARG;
  if (n_keys > 0 && (!keys || !pos1_out || !pos2_out || !count_out)) return CGCN_ERR_BAD_ARG;
  if (n_chroms < 1 || n_chroms > CGCN_PAIRS_MAX_CHROMS || resolution_bp < 8) return CGCN_ERR_UNSUPPORTED;
  ReducePlan p;
  if (!reduce_plan(n_keys, &p)) return CGCN_ERR_UNSUPPORTED;
  if (workspace_bytes < p.total) return CGCN_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (n_keys == 0) {
    if (hipMemsetAsync(chrom_offsets, 0, (size_t)(n_chroms + 1) * 8, st) != hipSuccess) return CGCN_ERR_LAUNCH;
    return hipMemsetAsync(n_records, 0, 8, st) == hipSuccess ? CGCN_OK : CGCN_ERR_LAUNCH;
  }
  char* w = ws_base(workspace);
  u64* sorted = (u64*)(w + p.o_sorted);
  size_t temp = p.temp;
  if (rocprim::radix_sort_keys((void*)(w + p.o_temp), temp, (const u64*)keys, sorted, (size_t)n_keys, 1u, 63u, st) != hipSuccess)
    return CGCN_ERR_LAUNCH;
  hipLaunchKernelGGL(k_pairs_heads<false>, dim3((unsigned)p.tiles), dim3(RED_THREADS), 0, st, n_keys, (const u64*)sorted,
                     (int*)(w + p.o_counts), (const long long*)nullptr, (const long long*)nullptr, n_chroms, (unsigned)resolution_bp,
                     (int*)nullptr, (int*)nullptr, (unsigned*)nullptr, (long long*)nullptr);
  hipLaunchKernelGGL(k_tile_scan<>, dim3(1), dim3(1024), 0, st, (int)p.tiles, (const int*)(w + p.o_counts), (long long*)(w + p.o_off),
                     n_records, (int*)nullptr, 0ll);
  hipLaunchKernelGGL(k_pairs_heads<true>, dim3((unsigned)p.tiles), dim3(RED_THREADS), 0, st, n_keys, (const u64*)sorted, (int*)nullptr,
                     (const long long*)(w + p.o_off), (const long long*)n_records, n_chroms, (unsigned)resolution_bp, pos1_out, pos2_out,
                     (unsigned*)(w + p.o_first), chrom_offsets);
  hipLaunchKernelGGL(k_pairs_counts, dim3((unsigned)((n_keys + RED_THREADS - 1) / RED_THREADS)), dim3(RED_THREADS), 0, st, n_keys,
                     (const long long*)n_records, (const unsigned*)(w + p.o_first), count_out);
  return launch_status();
}

}  // extern "C"
