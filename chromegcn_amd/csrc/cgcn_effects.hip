// chromegcn_amd/csrc/cgcn_effects.hip
//
// Window effects through the Hi-C graph (chromegcn_amd/effects.py): variant m replaces the input row
// of window u = windows[m] by alt[m] in both strands; the eval forward then changes, in layer 1, on u and on the rows that
// have u as a neighbour -- the variant's INSTANCES: instance 0 is u, then every v != u with a stored A[v, u] in the stored
// order of row u of the transpose.  From the unperturbed forward's saved aggregation H^k and layer inputs X^k:
//   k_eff_plan   per variant: its instance count and the position of the stored diagonal in the transposed row
//   k_eff_rows1  layer-1 instance rows  H_inst = H^1[v] + row_scale[v] val_t (alt - X^0[u])  (one fused multiply-add per
//                element, no gather), the residual input (alt for instance 0, X^0[v] otherwise) and the window of every row
//   k_eff_rows2  layer-2 instance rows  H_inst2 = H^2[v] + row_scale[v] sum_w val[v, w] (X1_inst[w's instance] - X^1[w])
//                over the stored entries w of row v that are instances of the same variant, in ascending w
// The dense gated part of both layers is cgcn_layer_fwd's row-local route on the instance tables (H_in given), the head
// cgcn_head_logits.  Instance tables are [S][rows][d]: ordinary feature tables with n = rows.
// One wavefront owns an instance: at d = 256 one wave per (instance, strand) row, at d = 128 one wave takes both strands'
// rows in its two halves; a lane holds 4 consecutive floats.  The window of a wave is wave-uniform, so the index walk of
// k_eff_rows2 takes 64 stored entries at a time, one per lane (each lane decides membership by binary search in the
// variant's sorted transposed row), and the members are then added in lane order = ascending w.  No atomics: every result
// is the same bits from run to run.
#include "cgcn_common.hpp"

#define EFF_NT 256   // threads of every kernel here
#define EFF_S 2      // strands: a variant always replaces both

// position of key in the sorted, duplicate-free list a[0 .. len), or -1
__device__ __forceinline__ int eff_find(const int* __restrict__ a, int len, int key) {
  int lo = 0, hi = len;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return (lo < len && a[lo] == key) ? lo : -1;
}

// the variant m < n_var with offsets[m] <= g < offsets[m + 1] (offsets strictly increasing: every variant has instance 0)
__device__ __forceinline__ int eff_variant(const long long* __restrict__ offsets, int n_var, long long g) {
  int lo = 0, hi = n_var;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= g) lo = mid;
    else hi = mid;
  }
  return lo;
}

// (instance, strand, first column) of this lane; false past the table
template <int D>
__device__ __forceinline__ bool eff_place(long long n_rows, long long& i, int& s, int& c0) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long long wave = (long long)blockIdx.x * (EFF_NT / WAVE) + __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  if (D == 256) {
    i = wave >> 1;
    s = (int)(wave & 1);
    c0 = lane * 4;
  } else {
    i = wave;
    s = lane >> 5;
    c0 = (lane & 31) * 4;
  }
  return i < n_rows;
}

// Row i of a table is instance (m, k): own != 0: instance 0 of variant i; else the instance offsets[0] + i of the batch.
// Fills u = windows[m], dp = diag_pos[m], the transposed row (tp0, tlen) and v, the instance's window, with the position j
// of (v, u) in the transposed row (-1: instance 0 without a stored diagonal).  false: not an instance (nothing is written).
__device__ __forceinline__ bool eff_instance(int n, const int* __restrict__ rowptr_t, const int* __restrict__ col_t,
                                             const int* __restrict__ windows, const long long* __restrict__ offsets,
                                             const int* __restrict__ diag_pos, int n_var, int own, long long i, int& m, int& k,
                                             int& u, int& dp, int& tp0, int& tlen, int& v, int& j) {
  if (own) {
    if (i >= n_var) return false;
    m = (int)i;
    k = 0;
  } else {
    const long long g = offsets[0] + i;
    m = eff_variant(offsets, n_var, g);
    if (g >= offsets[m + 1]) return false;
    k = (int)(g - offsets[m]);
  }
  u = windows[m];
  if ((unsigned)u >= (unsigned)n) return false;
  dp = diag_pos[m];
  tp0 = rowptr_t[u];
  tlen = rowptr_t[u + 1] - tp0;
  if (k == 0) {
    v = u;
    j = dp;
  } else {
    j = k - 1;
    if (dp >= 0 && j >= dp) ++j;
    if (j >= tlen) return false;
    v = col_t[tp0 + j];
  }
  return (unsigned)v < (unsigned)n;
}

__global__ __launch_bounds__(EFF_NT) void k_eff_plan(int n, const int* __restrict__ rowptr_t, const int* __restrict__ col_t,
                                                     int n_var, const int* __restrict__ windows, int* __restrict__ counts,
                                                     int* __restrict__ diag_pos) {
  const int m = blockIdx.x * EFF_NT + threadIdx.x;
  if (m >= n_var) return;
  const int u = windows[m];
  if ((unsigned)u >= (unsigned)n) {   // (the caller rejects these; never read outside the graph)
    counts[m] = 1;
    diag_pos[m] = -1;
    return;
  }
  const int p0 = rowptr_t[u], len = rowptr_t[u + 1] - p0;
  const int dp = eff_find(col_t + p0, len, u);
  counts[m] = len + (dp < 0 ? 1 : 0);
  diag_pos[m] = dp;
}

template <int D>
__global__ __launch_bounds__(EFF_NT) void k_eff_rows1(int n, const int* __restrict__ rowptr_t, const int* __restrict__ col_t,
                                                      const float* __restrict__ val_t, const float* __restrict__ row_scale,
                                                      const float* __restrict__ X0, const float* __restrict__ H1,
                                                      const int* __restrict__ windows, const float* __restrict__ alt,
                                                      const long long* __restrict__ offsets, const int* __restrict__ diag_pos,
                                                      int n_var, int own, int n_inst, float* __restrict__ H_inst,
                                                      float* __restrict__ X_inst, int* __restrict__ rows) {
  long long i;
  int s, c0, m, k, u, dp, tp0, tlen, v, j;
  if (!eff_place<D>(n_inst, i, s, c0)) return;
  if (!eff_instance(n, rowptr_t, col_t, windows, offsets, diag_pos, n_var, own, i, m, k, u, dp, tp0, tlen, v, j)) return;
  const f32x4 av = *(const f32x4*)(alt + ((size_t)m * EFF_S + s) * D + c0);
  const f32x4 xu = *(const f32x4*)(X0 + ((size_t)s * n + u) * D + c0);
  f32x4 h = *(const f32x4*)(H1 + ((size_t)s * n + v) * D + c0);
  if (j >= 0) {   // (instance 0 without a stored diagonal: H^1[u] unchanged)
    const float c = (row_scale ? row_scale[v] : 1.f) * (val_t ? val_t[tp0 + j] : 1.f);
#pragma unroll
    for (int e = 0; e < 4; ++e) h[e] = fmaf(c, av[e] - xu[e], h[e]);
  }
  const f32x4 xr = k == 0 ? av : *(const f32x4*)(X0 + ((size_t)s * n + v) * D + c0);
  const size_t o = ((size_t)s * n_inst + (size_t)i) * D + c0;
  *(f32x4*)(H_inst + o) = h;
  *(f32x4*)(X_inst + o) = xr;
  if (rows && s == 0 && (threadIdx.x & (WAVE - 1)) == 0) rows[i] = v;
}

template <int D>
__global__ __launch_bounds__(EFF_NT) void k_eff_rows2(int n, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                      const float* __restrict__ val, const float* __restrict__ row_scale,
                                                      const int* __restrict__ rowptr_t, const int* __restrict__ col_t,
                                                      const float* __restrict__ X1, const float* __restrict__ H2,
                                                      const int* __restrict__ windows, const long long* __restrict__ offsets,
                                                      const int* __restrict__ diag_pos, int n_var, int own, int n_inst,
                                                      int n_out, const float* __restrict__ X1_inst, float* __restrict__ H_out,
                                                      float* __restrict__ X_res) {
  long long r;
  int s, c0, m, k, u, dp, tp0, tlen, v, j;
  if (!eff_place<D>(n_out, r, s, c0)) return;
  if (!eff_instance(n, rowptr_t, col_t, windows, offsets, diag_pos, n_var, own, r, m, k, u, dp, tp0, tlen, v, j)) return;
  const long long io = offsets[m] - offsets[0];   // the variant's instance 0 in the layer-1 table
  const long long cnt = offsets[m + 1] - offsets[m];
  if (io < 0 || io + cnt > n_inst) return;
  const int lane = threadIdx.x & (WAVE - 1);
  const int* trow = col_t + tp0;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const int q1 = rowptr[v + 1];
  for (int q = rowptr[v]; q < q1; q += WAVE) {
    const int qq = q + lane;
    int w = -1, idx = -1;
    float wv = 0.f;
    if (qq < q1) {
      w = col[qq];
      wv = val ? val[qq] : 1.f;
      if (w == u) {
        idx = 0;
      } else {
        const int p = eff_find(trow, tlen, w);
        if (p >= 0) idx = 1 + p - ((dp >= 0 && p > dp) ? 1 : 0);
      }
      if (idx >= cnt || (unsigned)w >= (unsigned)n) idx = -1;
    }
    unsigned long long mask = __ballot(idx >= 0);
    while (mask) {   // the members of this chunk, in lane order = ascending w
      const int b = __builtin_ctzll(mask);
      mask &= mask - 1;
      const int wi = rl_i(w, b), ii = rl_i(idx, b);
      const float wf = rl_f(wv, b);
      const f32x4 xi = *(const f32x4*)(X1_inst + ((size_t)s * n_inst + (size_t)(io + ii)) * D + c0);
      const f32x4 x1 = *(const f32x4*)(X1 + ((size_t)s * n + wi) * D + c0);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = fmaf(wf, xi[e] - x1[e], acc[e]);
    }
  }
  f32x4 h = *(const f32x4*)(H2 + ((size_t)s * n + v) * D + c0);
  const float rs = row_scale ? row_scale[v] : 1.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) h[e] = fmaf(rs, acc[e], h[e]);
  const size_t o = ((size_t)s * n_out + (size_t)r) * D + c0;
  *(f32x4*)(H_out + o) = h;
  if (X_res) *(f32x4*)(X_res + o) = *(const f32x4*)(X1_inst + ((size_t)s * n_inst + (size_t)(io + k)) * D + c0);
}

static inline size_t eff_align(size_t b) { return (b + 255) & ~(size_t)255; }
static inline bool eff_dim_ok(int S, int d) { return S == EFF_S && (d == 128 || d == 256); }
#define EFF_MAX_ROWS (1 << 28)   // rows of an instance table: the grid and every 32-bit count stay in range
static inline unsigned eff_blocks(int rows, int d) {
  const long long waves = (long long)rows * (d == 256 ? 2 : 1);
  return (unsigned)((waves + EFF_NT / WAVE - 1) / (EFF_NT / WAVE));
}

extern "C" {

size_t cgcn_effects_workspace_bytes(int n_inst, int S, int d, int layers) {
  if (n_inst < 0 || n_inst > EFF_MAX_ROWS || layers < 1 || layers > 2 || !eff_dim_ok(S, d)) return 0;
  const size_t feat = eff_align((size_t)n_inst * S * d * sizeof(float));
  return (size_t)(2 + layers) * feat + eff_align((size_t)n_inst * S * sizeof(float));
}

int cgcn_effects_plan(cgcn_stream_t stream, int n, const int32_t* rowptr_t, const int32_t* col_t, int n_var,
                      const int32_t* windows, int32_t* counts, int32_t* diag_pos) {
  if (n < 0 || n_var < 0) return CGCN_ERR_BAD_ARG;
  if (!rowptr_t || !col_t || !windows || !counts || !diag_pos) return CGCN_ERR_BAD_ARG;
  if (n_var == 0) return CGCN_OK;
  hipLaunchKernelGGL(k_eff_plan, dim3((n_var + EFF_NT - 1) / EFF_NT), dim3(EFF_NT), 0, (hipStream_t)stream, n, rowptr_t, col_t,
                     n_var, windows, counts, diag_pos);
  return launch_status();
}

int cgcn_effects_rows1(cgcn_stream_t stream, int n, int S, int d, const int32_t* rowptr_t, const int32_t* col_t,
                       const float* val_t, const float* row_scale, const float* X0, const float* H1, const int32_t* windows,
                       const float* alt, const long long* offsets, const int32_t* diag_pos, int n_var, int own, int n_inst,
                       float* H_inst, float* X_inst, int32_t* rows) {
  if (n < 0 || n_var < 0 || n_inst < 0) return CGCN_ERR_BAD_ARG;
  if (!eff_dim_ok(S, d) || n_inst > EFF_MAX_ROWS) return CGCN_ERR_UNSUPPORTED;
  if (!rowptr_t || !col_t || !X0 || !H1 || !windows || !alt || !offsets || !diag_pos || !H_inst || !X_inst)
    return CGCN_ERR_BAD_ARG;
  if (misaligned16(X0) || misaligned16(H1) || misaligned16(alt) || misaligned16(H_inst) || misaligned16(X_inst))
    return CGCN_ERR_BAD_ARG;
  if (own && n_inst != n_var) return CGCN_ERR_BAD_ARG;
  if (n_inst == 0 || n_var == 0) return CGCN_OK;
  hipStream_t st = (hipStream_t)stream;
  if (d == 128)
    hipLaunchKernelGGL(k_eff_rows1<128>, dim3(eff_blocks(n_inst, d)), dim3(EFF_NT), 0, st, n, rowptr_t, col_t, val_t, row_scale,
                       X0, H1, windows, alt, offsets, diag_pos, n_var, own, n_inst, H_inst, X_inst, rows);
  else
    hipLaunchKernelGGL(k_eff_rows1<256>, dim3(eff_blocks(n_inst, d)), dim3(EFF_NT), 0, st, n, rowptr_t, col_t, val_t, row_scale,
                       X0, H1, windows, alt, offsets, diag_pos, n_var, own, n_inst, H_inst, X_inst, rows);
  return launch_status();
}

int cgcn_effects_rows2(cgcn_stream_t stream, int n, int S, int d, const int32_t* rowptr, const int32_t* col, const float* val,
                       const float* row_scale, const int32_t* rowptr_t, const int32_t* col_t, const float* X1, const float* H2,
                       const int32_t* windows, const long long* offsets, const int32_t* diag_pos, int n_var, int own, int n_inst,
                       const float* X1_inst, float* H_out, float* X_res) {
  if (n < 0 || n_var < 0 || n_inst < 0) return CGCN_ERR_BAD_ARG;
  if (!eff_dim_ok(S, d) || n_inst > EFF_MAX_ROWS) return CGCN_ERR_UNSUPPORTED;
  if (!rowptr || !col || !rowptr_t || !col_t || !X1 || !H2 || !windows || !offsets || !diag_pos || !X1_inst || !H_out)
    return CGCN_ERR_BAD_ARG;
  if (misaligned16(X1) || misaligned16(H2) || misaligned16(X1_inst) || misaligned16(H_out) || (X_res && misaligned16(X_res)))
    return CGCN_ERR_BAD_ARG;
  if (own && !X_res) return CGCN_ERR_BAD_ARG;   // the read-out rows are not the layer-1 table's: they need their own residual
  if (H_out == X1_inst || X_res == X1_inst) return CGCN_ERR_BAD_ARG;
  const int n_out = own ? n_var : n_inst;
  if (n_out == 0 || n_var == 0) return CGCN_OK;
  hipStream_t st = (hipStream_t)stream;
  if (d == 128)
    hipLaunchKernelGGL(k_eff_rows2<128>, dim3(eff_blocks(n_out, d)), dim3(EFF_NT), 0, st, n, rowptr, col, val, row_scale, rowptr_t,
                       col_t, X1, H2, windows, offsets, diag_pos, n_var, own, n_inst, n_out, X1_inst, H_out, X_res);
  else
    hipLaunchKernelGGL(k_eff_rows2<256>, dim3(eff_blocks(n_out, d)), dim3(EFF_NT), 0, st, n, rowptr, col, val, row_scale, rowptr_t,
                       col_t, X1, H2, windows, offsets, diag_pos, n_var, own, n_inst, n_out, X1_inst, H_out, X_res);
  return launch_status();
}

}  // extern "C"
