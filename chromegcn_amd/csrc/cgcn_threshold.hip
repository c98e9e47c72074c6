// chromegcn_amd/csrc/cgcn_threshold.hip -- thresholded multi-label counts: everything the five
// binary-relevance metrics of utils/metrics.py:29-109 (ACC, HA, ebF1, miF1, maF1) need, as integers, for T thresholds
// per label in one stream over probs and targets.
//
//   Y[i][c] = targets[i][c] > 0.5f          P[t][i][c] = probs[i][c] >= thresholds[t][c]   (float32; a NaN is never predicted)
//
// k_threshold_rows<CH, TT, NLD>.  A workgroup owns a contiguous block of rows and a group of thresholds.
//   * Rows reach the CU in TILES: the rows of a workgroup are one contiguous stretch of memory, so all its threads fetch the
//     next tile as flat coalesced dwords (whatever C is: 103 labels are 412-byte rows) into registers while the current tile
//     is counted, and hand it over through LDS -- a tile is the bytes in flight, not a row.
//   * Counting: lane <-> label, a wave takes a row in CH chunks of 64 labels and owns TT thresholds; the waves of a TEAM
//     own consecutive groups of TT thresholds and count the SAME rows from LDS (a workgroup of 8 waves has 8 / waves-per-team
//     teams, which take the rows of a tile in turn and share the histograms), so that everything a wave
//     accumulates stays in registers whatever T is: the thresholds of its labels th[TT][CH], and per (threshold, label) the
//     rows with P and the rows with P and Y, 16 bits each in one register cnt[TT][CH].
//   * A v_cmp IS the 64-bit ballot of its chunk: the popcounts |P|, |P & Y|, |Y| are scalar work.  The row's record of
//     threshold j, k = |P| + |Y| and |P & Y|, goes packed into lane 4j (one DPP move); after the TT thresholds these lanes
//     add into the workgroup's LDS histogram rows / tpsum [threshold][k] -- different lanes hold different thresholds, so a
//     wave never meets itself on a word.  The row is exact iff k == 2 |P & Y| (|P & Y| <= min(|P|, |Y|)).
// Workgroup totals leave through 64-bit integer atomics on the outputs, which k_threshold_zero has cleared (zero partials
// are skipped: most of the 2C + 1 bins of a histogram stay empty).  Integer addition is associative: the same bits whatever
// the grid or the arrival order.
//
// Bounds.  A workgroup takes at most 65 535 rows (threshold_plan): the two per-label counts of a (threshold, label) share one
// register, 16 bits each (tp <= pp <= rows: no carry between the halves), and an LDS word (uint32) holds at most
// rows * C < 2^16 * 2^10 = 2^26; the totals are 64-bit.
// LDS (64 KiB per workgroup): 2 (2C + 1) words per threshold the workgroup owns, the rest (>= 8 KiB) is the tile.  A
// workgroup owns as many thresholds as fit (34 at C = 103) and the grid's y dimension walks the thresholds in such groups:
// at large C * T every group streams the rows again (from L2 / the Infinity Cache for all but the first) -- the slow route,
// cgcn_debug_threshold_route() > 1.
#include "cgcn_common.hpp"

namespace {

typedef unsigned long long u64;

constexpr int THR_MAX_C = 1024, THR_MAX_T = 64;
constexpr int THR_MAX_WAVES = 8;                 // __launch_bounds__(512): 256 registers per lane
constexpr long long THR_MAX_ROWS = 65535;        // rows per workgroup (see Bounds)
constexpr size_t THR_LDS_BYTES = 65536;          // dynamic LDS of a launch
constexpr size_t THR_TILE_MIN_BYTES = 8192;      // ... of which the tile gets at least this: one row of 1024 labels
constexpr long long THR_MIN_ROWS = 128;       // ... and at least these: a workgroup's flush is ~12 000 atomics whatever it counted
constexpr int THR_GRID_X = 512;                  // two workgroups per CU: every partial is one atomic more

struct ThresholdPlan {
  int CH, TT, NLD;         // kernel instance: chunks of 64 labels, thresholds per wave, tile dwords per thread and array
  int waves, TW, groups;   // waves per team, thresholds per workgroup (waves * TT), groups of TW thresholds (grid y)
  int teams;               // teams of `waves` waves per workgroup: team k counts rows k, k + teams, ... of every tile
  int tile_rows;
  long long rows_per_wg;
  unsigned grid_x;
  size_t hist_bytes, lds;
};

// false: unsupported shape
bool threshold_plan(long long n, int C, int T, ThresholdPlan& p) {
  if (n < 1 || C < 1 || C > THR_MAX_C || T < 1 || T > THR_MAX_T) return false;
  const int ch = (C + 63) / 64;
  if (ch <= 4) { p.CH = ch; p.TT = 8; p.NLD = 8; } else if (ch <= 8) { p.CH = 8; p.TT = 4; p.NLD = 8; } else { p.CH = 16; p.TT = 2; p.NLD = 16; }
  const size_t per_t = (size_t)2 * (2 * C + 1) * sizeof(uint32_t);
  const int fit = (int)((THR_LDS_BYTES - THR_TILE_MIN_BYTES) / per_t);   // >= 3 (C = 1024: 16 392 bytes per threshold)
  int waves = (T + p.TT - 1) / p.TT;
  if (waves > THR_MAX_WAVES) waves = THR_MAX_WAVES;
  if (waves > fit / p.TT) waves = fit / p.TT;            // >= 1: TT <= fit for every instance
  p.waves = waves;
  p.teams = THR_MAX_WAVES / waves;
  p.TW = waves * p.TT;
  p.groups = (T + p.TW - 1) / p.TW;
  p.hist_bytes = (size_t)(p.TW < T ? p.TW : T) * per_t;
  // a tile: what the threads can hold in flight (64 waves teams NLD dwords per array) and what the LDS has left, in whole rows
  long long tile = (long long)64 * waves * p.teams * p.NLD / C;    // >= 1: 64 NLD >= 64 CH >= C
  const long long room = (long long)((THR_LDS_BYTES - p.hist_bytes) / ((size_t)8 * C));   // >= 1: 8 C <= 8 192
  if (tile > room) tile = room;
  p.tile_rows = (int)tile;
  p.lds = p.hist_bytes + (size_t)tile * C * 8;
  long long rows = (n + THR_GRID_X - 1) / THR_GRID_X;
  if (rows < THR_MIN_ROWS) rows = THR_MIN_ROWS;
  if (rows > THR_MAX_ROWS) rows = THR_MAX_ROWS;
  const long long gx = (n + rows - 1) / rows;
  if (gx > 2147483647ll) return false;                   // n >= 2^47
  p.rows_per_wg = rows;
  p.grid_x = (unsigned)gx;
  return true;
}

__global__ void k_threshold_zero(int C, int T, u64* __restrict__ pos, u64* __restrict__ tp, u64* __restrict__ pp,
                                 u64* __restrict__ exact, u64* __restrict__ rows, u64* __restrict__ tpsum) {
  const int K = 2 * C + 1;
  const int stride = gridDim.x * blockDim.x;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < T * K; i += stride) {
    rows[i] = 0;
    tpsum[i] = 0;
    if (i < T * C) { tp[i] = 0; pp[i] = 0; }
    if (i < C) pos[i] = 0;
    if (i < T) exact[i] = 0;
  }
}

// v[J] into lanes 4J .. 4J + 3 of rec for every J: one DPP move each (identity quad_perm, row J / 4, bank J % 4)
template <int J, int TT>
__device__ __forceinline__ int place_records(int rec, const int (&v)[TT]) {
  if constexpr (J < TT) {
    rec = __builtin_amdgcn_update_dpp(rec, v[J], 0xE4, 1 << (J >> 2), 1 << (J & 3), false);
    return place_records<J + 1, TT>(rec, v);
  } else {
    return rec;
  }
}

// packed row record of one threshold: bits 0-11 k = |P| + |Y| (<= 2048), bits 12-22 |P & Y| (<= 1024)
template <int CH, int TT, int NLD>
__global__ __launch_bounds__(THR_MAX_WAVES * 64) void k_threshold_rows(
    long long n, int C, int T, int TW, int W, int tile_rows, int hist_words, long long rows_per_wg,
    const float* __restrict__ probs, const float* __restrict__ targets, const float* __restrict__ thr,
    u64* __restrict__ pos, u64* __restrict__ tp, u64* __restrict__ pp, u64* __restrict__ exact, u64* __restrict__ rows,
    u64* __restrict__ tpsum) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  uint32_t* const hist = lds;                               // [threshold of the workgroup][rows | tpsum][K]
  float* const sp = (float*)(lds + hist_words);             // the tile: [tile_rows][C] probabilities
  float* const sy = sp + (size_t)tile_rows * C;             //           [tile_rows][C] targets
  const int lane = threadIdx.x & 63;
  const int wave_wg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int team = wave_wg / W, wave = wave_wg - team * W, teams = (int)(blockDim.x >> 6) / W;
  const int NT = blockDim.x;
  const int K = 2 * C + 1;
  const int tg0 = blockIdx.y * TW;                  // the workgroup's thresholds: [tg0, tg0 + ntg)
  const int ntg = min(TW, T - tg0);
  const int t0 = tg0 + wave * TT;                   // the wave's: [t0, t0 + nt), none for a spare wave of the last group
  const int nt = max(0, min(TT, tg0 + ntg - t0));
  for (int i = threadIdx.x; i < ntg * 2 * K; i += NT) hist[i] = 0;

  const float nanf_ = __builtin_nanf("");
  float th[TT][CH];        // a spare slot (j >= nt) or label (c >= C) holds NaN: never predicted, nothing of it is kept
  uint32_t cnt[TT][CH];    // rows with P in the low half, rows with P and Y in the high half
  uint32_t cpos[CH];
#pragma unroll
  for (int ch = 0; ch < CH; ++ch) {
    const int c = ch * 64 + lane;
    cpos[ch] = 0;
#pragma unroll
    for (int j = 0; j < TT; ++j) {
      th[j][ch] = (j < nt && c < C) ? thr[(size_t)(t0 + j) * C + c] : nanf_;
      cnt[j][ch] = 0;
    }
  }
  uint32_t cexact = 0;
  const bool owner = (lane & 3) == 0 && (lane >> 2) < nt;   // lane 4j keeps the row statistics of the wave's threshold j
  uint32_t* const my_hist = hist + (size_t)(wave * TT + (lane >> 2)) * 2 * K;   // owners only

  const long long r0 = (long long)blockIdx.x * rows_per_wg;
  const long long r1 = min(n, r0 + rows_per_wg);
  const float* const gp = probs + (size_t)r0 * C;
  const float* const gy = targets + (size_t)r0 * C;
  const long long total = (r1 - r0) * C;            // elements of the workgroup's stretch: < 2^16 * 2^10
  const int tile_elems = tile_rows * C;             // <= NT * NLD
  float fp[NLD], fy[NLD];                           // the next tile, in flight
#pragma unroll
  for (int i = 0; i < NLD; ++i) {
    const int e = threadIdx.x + i * NT;
    const bool in = e < tile_elems && e < total;
    fp[i] = in ? gp[e] : 0.f;
    fy[i] = in ? gy[e] : 0.f;
  }
  for (long long base = 0; base < total; base += tile_elems) {
    __syncthreads();                                // the previous tile has been counted (first trip: hist is cleared)
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int e = threadIdx.x + i * NT;
      if (e < tile_elems) {
        sp[e] = fp[i];
        sy[e] = fy[i];
      }
    }
    __syncthreads();
    const long long next = base + tile_elems;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int e = threadIdx.x + i * NT;
      const bool in = e < tile_elems && next + e < total;
      fp[i] = in ? gp[next + e] : 0.f;
      fy[i] = in ? gy[next + e] : 0.f;
    }
    if (nt == 0) continue;                          // a spare wave only carries tiles
    const int nrows = (int)(min((long long)tile_elems, total - base) / C);
    for (int rr = team; rr < nrows; rr += teams) {
      const float* const rp = sp + rr * C;
      const float* const ry = sy + rr * C;
      int ny = 0, np[TT], ntp[TT];                  // scalars: the row's |Y|, and |P|, |P & Y| of each threshold of the wave
#pragma unroll
      for (int j = 0; j < TT; ++j) {
        np[j] = 0;
        ntp[j] = 0;
      }
#pragma unroll
      for (int ch = 0; ch < CH; ++ch) {
        const int c = ch * 64 + lane;
        const float p = c < C ? rp[c] : nanf_;
        const bool y = c < C ? ry[c] > 0.5f : false;
        const u64 Yb = __ballot(y);
        ny += __popcll(Yb);
        cpos[ch] += y ? 1u : 0u;
        const uint32_t inc = y ? 0x10001u : 1u;
#pragma unroll
        for (int j = 0; j < TT; ++j) {
          const bool pred = p >= th[j][ch];
          const u64 P = __ballot(pred);
          cnt[j][ch] += pred ? inc : 0u;
          np[j] += __popcll(P);
          ntp[j] += __popcll(P & Yb);
        }
      }
      int recs[TT];
#pragma unroll
      for (int j = 0; j < TT; ++j) recs[j] = (np[j] + ny) | (ntp[j] << 12);
      const int rec = place_records<0, TT>(0, recs);
      if (owner) {
        const int k = rec & 0xfff, both = rec >> 12;
        cexact += k == 2 * both ? 1u : 0u;
        atomicAdd(&my_hist[k], 1u);
        if (both) atomicAdd(&my_hist[K + k], (uint32_t)both);
      }
    }
  }
  if (nt > 0) {
#pragma unroll
    for (int j = 0; j < TT; ++j) {
      if (j < nt) {
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) {
          const int c = ch * 64 + lane;
          if (c < C) {
            if (cnt[j][ch] & 0xffffu) atomicAdd(&pp[(size_t)(t0 + j) * C + c], (u64)(cnt[j][ch] & 0xffffu));
            if (cnt[j][ch] >> 16) atomicAdd(&tp[(size_t)(t0 + j) * C + c], (u64)(cnt[j][ch] >> 16));
          }
        }
      }
    }
    if (owner && cexact) atomicAdd(&exact[t0 + (lane >> 2)], (u64)cexact);
    if (wave == 0 && blockIdx.y == 0) {
#pragma unroll
      for (int ch = 0; ch < CH; ++ch) {
        const int c = ch * 64 + lane;
        if (c < C && cpos[ch]) atomicAdd(&pos[c], (u64)cpos[ch]);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ntg * K; i += NT) {
    const int tl = i / K, k = i - tl * K;
    const uint32_t a = hist[(size_t)tl * 2 * K + k], b = hist[(size_t)tl * 2 * K + K + k];
    if (a) atomicAdd(&rows[(size_t)(tg0 + tl) * K + k], (u64)a);
    if (b) atomicAdd(&tpsum[(size_t)(tg0 + tl) * K + k], (u64)b);
  }
}

template <int CH, int TT, int NLD>
void launch_threshold_rows(hipStream_t st, const ThresholdPlan& p, long long n, int C, int T, const float* probs,
                           const float* targets, const float* thr, u64* pos, u64* tp, u64* pp, u64* exact, u64* rows,
                           u64* tpsum) {
  hipLaunchKernelGGL((k_threshold_rows<CH, TT, NLD>), dim3(p.grid_x, p.groups), dim3(p.waves * p.teams * 64), p.lds, st, n, C, T, p.TW,
                     p.waves, p.tile_rows, (int)(p.hist_bytes / sizeof(uint32_t)), p.rows_per_wg, probs, targets, thr, pos, tp, pp,
                     exact, rows, tpsum);
}

}  // namespace

extern "C" {

// The kernels accumulate straight into the outputs and keep nothing between calls: the workspace is reserved (a non-zero size,
// so that 0 keeps meaning "unsupported shape") and is not written.
size_t cgcn_threshold_workspace_bytes(long long n, int C, int T) {
  ThresholdPlan p;
  return threshold_plan(n, C, T, p) ? 256 : 0;
}

int cgcn_debug_threshold_route(long long n, int C, int T) {
  ThresholdPlan p;
  return threshold_plan(n, C, T, p) ? p.groups : CGCN_ERR_UNSUPPORTED;
}

int cgcn_threshold_counts(cgcn_stream_t stream, long long n, int C, int T, const float* probs, const float* targets,
                          const float* thresholds, long long* pos, long long* tp, long long* pp, long long* exact,
                          long long* rows, long long* tpsum, void* workspace, size_t workspace_bytes) {
  if (!probs || !targets || !thresholds || !pos || !tp || !pp || !exact || !rows || !tpsum || !workspace)
    return CGCN_ERR_BAD_ARG;
  ThresholdPlan p;
  if (!threshold_plan(n, C, T, p)) return CGCN_ERR_UNSUPPORTED;
  if (workspace_bytes < cgcn_threshold_workspace_bytes(n, C, T)) return CGCN_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  u64 *o_pos = (u64*)pos, *o_tp = (u64*)tp, *o_pp = (u64*)pp, *o_exact = (u64*)exact, *o_rows = (u64*)rows,
      *o_tpsum = (u64*)tpsum;
  const int cells = T * (2 * C + 1);
  hipLaunchKernelGGL(k_threshold_zero, dim3((cells + 255) / 256 < 256 ? (cells + 255) / 256 : 256), dim3(256), 0, st, C, T,
                     o_pos, o_tp, o_pp, o_exact, o_rows, o_tpsum);
#define THR_LAUNCH(CH_, TT_, NLD_) \
  launch_threshold_rows<CH_, TT_, NLD_>(st, p, n, C, T, probs, targets, thresholds, o_pos, o_tp, o_pp, o_exact, o_rows, o_tpsum)
  switch (p.CH) {
    case 1: THR_LAUNCH(1, 8, 8); break;
    case 2: THR_LAUNCH(2, 8, 8); break;
    case 3: THR_LAUNCH(3, 8, 8); break;
    case 4: THR_LAUNCH(4, 8, 8); break;
    case 8: THR_LAUNCH(8, 4, 8); break;
    default: THR_LAUNCH(16, 2, 16); break;
  }
#undef THR_LAUNCH
  return launch_status();
}

}  // extern "C"
