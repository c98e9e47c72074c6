// chromegcn_amd/csrc/cgcn_tsne.hip
//
// Exact (O(n^2)) t-SNE of n points into the plane, as scikit-learn defines it with method='exact' (DESIGN.md section 4.7;
// the contract of every entry point is stated in include/chromegcn.h above cgcn_tsne_sqdist).  Every n x n matrix is
// row-major fp32 with a row pitch `ld` (floats, a multiple of 4, >= n), so that rows can be read 16 bytes per lane.
//
//   k_tsne_sqdist       D[i,j] = sum_k (x_ik - x_jk)^2, 64 x 64 tiles, both row blocks through LDS in slices of 32 features;
//                       the difference form and one fixed order over k: D[i,i] = 0 and D[i,j] = D[j,i] bit for bit
//   k_tsne_affinities   one workgroup per row: the perplexity search in float64 on the fp32 row, re-read every step
//   k_tsne_rowsum       float64 sum of every row of C (stage one of the total; sum (C + C^T) = 2 sum C)
//   k_tsne_total        a fixed-order float64 sum of n partials by one workgroup (stage two; also Z of the gradient)
//   k_tsne_symmetrize   tile pairs (bi <= bj): P = max((C + C^T) / total, eps), the diagonal 0; safe in place
//   k_tsne_pass<0>      Z row partials: sum_{j != i} w_ij, fp32, Y staged in LDS in chunks of TG_CH columns
//   k_tsne_pass<1|2>    the hot loop: streams P once (16 bytes per lane), writes the gradient row (and the KL row partial)
//   k_tsne_update       gains / momentum step of the n x 2 state by one workgroup; finishes KL and the gradient norm
//
// No atomics: a row is reduced inside one wave, totals by one workgroup in a fixed order, so two launches with the same
// inputs give the same bits.
#include "cgcn_compact.hpp"

#include <math.h>

#define TS_EPS 2.220446049250313e-16   // numpy's float64 machine epsilon: scikit-learn's MACHINE_EPSILON
#define SQ_T 64                        // rows / columns of D per workgroup
#define SQ_K 32                        // features per LDS slice
#define TG_THREADS 256
#define TG_RW 2                        // rows of P per wave
#define TG_ROWS (TG_RW * TG_THREADS / WAVE)
#define TG_CH 2048                     // columns of Y per LDS chunk (16 KiB)
#define SUM_THREADS 1024

static inline bool ts_misaligned16(const void* p) { return ((uintptr_t)p & 15u) != 0; }

// ------------------------------------------------------------------------------------------
// squared distances
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tsne_sqdist(int n, int d, int ld, const float* __restrict__ X, float* __restrict__ D) {
  __shared__ float sa[SQ_T][SQ_K + 1], sb[SQ_T][SQ_K + 1];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int bi = blockIdx.y * SQ_T, bj = blockIdx.x * SQ_T;
  float acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
  for (int k0 = 0; k0 < d; k0 += SQ_K) {
    for (int t = tid; t < SQ_T * SQ_K / 4; t += 256) {
      const int r = t >> 3, c4 = (t & 7) * 4, k = k0 + c4;   // d % 4 == 0: k < d covers k + 3
      f32x4 va = {0.f, 0.f, 0.f, 0.f}, vb = {0.f, 0.f, 0.f, 0.f};
      if (k < d && bi + r < n) va = *(const f32x4*)(X + (size_t)(bi + r) * d + k);
      if (k < d && bj + r < n) vb = *(const f32x4*)(X + (size_t)(bj + r) * d + k);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        sa[r][c4 + q] = va[q];
        sb[r][c4 + q] = vb[q];
      }
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < SQ_K; ++k) {
      float a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] = sa[ty + 16 * r][k];
#pragma unroll
      for (int c = 0; c < 4; ++c) b[c] = sb[tx + 16 * c][k];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float df = a[r] - b[c];
          acc[r][c] = __builtin_fmaf(df, df, acc[r][c]);
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = bi + ty + 16 * r;
    if (i >= n) continue;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = bj + tx + 16 * c;
      if (j < n) D[(size_t)i * ld + j] = acc[r][c];
    }
  }
}

// ------------------------------------------------------------------------------------------
// conditional affinities: scikit-learn's _binary_search_perplexity, one row per workgroup
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tsne_affinities(int n, int ld, const float* __restrict__ D, double log_perp,
                                                         float* __restrict__ C, double* __restrict__ beta_out) {
  __shared__ double sh0[4], sh1[4];
  const int tid = threadIdx.x, i = blockIdx.x;
  const float* row = D + (size_t)i * ld;
  double beta = 1.0, beta_min = -INFINITY, beta_max = INFINITY, used = 1.0, total = 1.0;
  for (int step = 0; step < 100; ++step) {
    double s0 = 0.0, s1 = 0.0;
    for (int j = tid; j < n; j += 256) {
      if (j == i) continue;
      const double dd = (double)row[j], e = exp(-dd * beta);
      s0 += e;
      s1 += dd * e;
    }
    s0 = block_sum_d<4>(s0, sh0);
    s1 = block_sum_d<4>(s1, sh1);
    if (s0 == 0.0) s0 = 1e-8;
    used = beta;
    total = s0;
    const double diff = log(s0) + beta * (s1 / s0) - log_perp;
    if (fabs(diff) <= 1e-5) break;
    if (diff > 0.0) {
      beta_min = beta;
      beta = beta_max == INFINITY ? beta * 2.0 : (beta + beta_max) * 0.5;
    } else {
      beta_max = beta;
      beta = beta_min == -INFINITY ? beta * 0.5 : (beta + beta_min) * 0.5;
    }
  }
  float* out = C + (size_t)i * ld;
  for (int j = tid; j < n; j += 256) out[j] = j == i ? 0.f : (float)(exp(-(double)row[j] * used) / total);
  if (tid == 0) beta_out[i] = used;
}

// ------------------------------------------------------------------------------------------
// totals and symmetrisation
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tsne_rowsum(int n, int ld, const float* __restrict__ C, double* __restrict__ part) {
  __shared__ double sh[4];
  const float* row = C + (size_t)blockIdx.x * ld;
  double s = 0.0;
  for (int j = threadIdx.x; j < n; j += 256) s += (double)row[j];
  s = block_sum_d<4>(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

template <typename T>
__global__ __launch_bounds__(SUM_THREADS) void k_tsne_total(int n, const T* __restrict__ part, double scale, double* __restrict__ out) {
  __shared__ double sh[SUM_THREADS / WAVE];
  double s = 0.0;
  for (int t = threadIdx.x; t < n; t += SUM_THREADS) s += (double)part[t];
  s = block_sum_d<SUM_THREADS / WAVE>(s, sh);
  if (threadIdx.x == 0) out[0] = s * scale;
}

// tile pair (bi, bj), bi <= bj: both tiles are read into LDS before either is written, and no other workgroup touches them
__global__ __launch_bounds__(256) void k_tsne_symmetrize(int n, int ld, const float* C, float* P, const double* __restrict__ total) {
  const int bi = blockIdx.y * SQ_T, bj = blockIdx.x * SQ_T;
  if (bi > bj) return;
  __shared__ float sa[SQ_T][SQ_T + 1], sb[SQ_T][SQ_T + 1];
  const int tid = threadIdx.x;
  for (int t = tid; t < SQ_T * SQ_T; t += 256) {
    const int r = t >> 6, c = t & 63;
    sa[r][c] = (bi + r < n && bj + c < n) ? C[(size_t)(bi + r) * ld + bj + c] : 0.f;
    sb[r][c] = (bj + r < n && bi + c < n) ? C[(size_t)(bj + r) * ld + bi + c] : 0.f;
  }
  __syncthreads();
  const double tot = fmax(total[0], TS_EPS);
  for (int t = tid; t < SQ_T * SQ_T; t += 256) {
    const int r = t >> 6, c = t & 63;
    if (bi + r < n && bj + c < n) {
      const double v = ((double)sa[r][c] + (double)sb[c][r]) / tot;
      P[(size_t)(bi + r) * ld + bj + c] = bi + r == bj + c ? 0.f : (float)fmax(v, TS_EPS);
    }
    if (bi != bj && bj + r < n && bi + c < n) {
      const double v = ((double)sa[c][r] + (double)sb[r][c]) / tot;
      P[(size_t)(bj + r) * ld + bi + c] = (float)fmax(v, TS_EPS);
    }
  }
}

// ------------------------------------------------------------------------------------------
// the objective: Z, gradient, KL
// ------------------------------------------------------------------------------------------
// four consecutive columns j0 .. j0 + 3 of one row i.  TAIL: some of them are at or beyond n and count for nothing.
template <int MODE, bool TAIL>
__device__ __forceinline__ void tsne_quad(int n, int i, int j0, float yix, float yiy, const f32x4 xj, const f32x4 yj, const f32x4 p,
                                          float e, float zf, float invz, float& a0, float& a1, double& kl) {
  const float eps = (float)TS_EPS;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float dx = yix - xj[q], dy = yiy - yj[q];
    float w = __builtin_amdgcn_rcpf(1.f + __builtin_fmaf(dx, dx, dy * dy));
    float ep = MODE ? e * p[q] : 0.f;
    if (TAIL && j0 + q >= n) {
      w = 0.f;
      ep = 0.f;
    }
    if (MODE == 0) {
      a0 += j0 + q == i ? 0.f : w;
    } else {
      // w / Z from the reciprocal and one correction step (two fused multiply-adds): correctly rounded but for rare
      // last-bit cases, and exact whenever the quotient is representable (n = 2: Q = 1/2 = P, a gradient of exactly 0)
      const float q0 = w * invz;
      const float qq = fmaxf(__builtin_fmaf(__builtin_fmaf(-q0, zf, w), invz, q0), eps);
      const float m = (ep - qq) * w;
      a0 = __builtin_fmaf(m, dx, a0);
      a1 = __builtin_fmaf(m, dy, a1);
      if (MODE == 2) kl += (double)(ep * logf(fmaxf(ep, eps) / qq));
    }
  }
}

// MODE 0: zrow[i] = sum_{j != i} w_ij.  MODE 1: grad[i] = 4 sum_j (e P_ij - max(w_ij / Z, eps)) w_ij (y_i - y_j).
// MODE 2: the same gradient bits, and klrow[i] = sum_j e P_ij log(max(e P_ij, eps) / Q_ij).
template <int MODE>
__global__ __launch_bounds__(TG_THREADS) void k_tsne_pass(int n, int ld, const float* __restrict__ P, const float* __restrict__ Y,
                                                          float e, const double* __restrict__ Zp, float* __restrict__ zrow,
                                                          float* __restrict__ grad, double* __restrict__ klrow) {
  __shared__ __attribute__((aligned(16))) float sx[TG_CH];
  __shared__ __attribute__((aligned(16))) float sy[TG_CH];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
  const int r0 = blockIdx.x * TG_ROWS + wv * TG_RW;
  int row[TG_RW];
  float yix[TG_RW], yiy[TG_RW], a0[TG_RW], a1[TG_RW];
  double kl[TG_RW];
  const float* prow[TG_RW];
#pragma unroll
  for (int r = 0; r < TG_RW; ++r) {
    row[r] = r0 + r < n ? r0 + r : n - 1;   // a row beyond n repeats the last one and is not written
    yix[r] = Y[2 * row[r]];
    yiy[r] = Y[2 * row[r] + 1];
    prow[r] = P + (size_t)row[r] * ld;
    a0[r] = a1[r] = 0.f;
    kl[r] = 0.0;
  }
  float zf = 1.f, invz = 1.f;
  if (MODE) {
    zf = (float)Zp[0];
    invz = 1.f / zf;
  }
  for (int c0 = 0; c0 < n; c0 += TG_CH) {
    __syncthreads();
    for (int t = tid; t < TG_CH; t += TG_THREADS) {
      const int j = c0 + t;
      f32x2 v = {0.f, 0.f};
      if (j < n) v = *(const f32x2*)(Y + 2 * (size_t)j);
      sx[t] = v[0];
      sy[t] = v[1];
    }
    __syncthreads();
    const int cend = ld - c0 < TG_CH ? ld - c0 : TG_CH;   // a multiple of 4
    for (int c = lane * 4; c < cend; c += WAVE * 4) {
      const f32x4 xj = *(const f32x4*)(sx + c), yj = *(const f32x4*)(sy + c);
      f32x4 p[TG_RW];
#pragma unroll
      for (int r = 0; r < TG_RW; ++r) p[r] = MODE ? *(const f32x4*)(prow[r] + c0 + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
      const int j0 = c0 + c;
      if (j0 + 4 <= n) {
#pragma unroll
        for (int r = 0; r < TG_RW; ++r) tsne_quad<MODE, false>(n, row[r], j0, yix[r], yiy[r], xj, yj, p[r], e, zf, invz, a0[r], a1[r], kl[r]);
      } else {
#pragma unroll
        for (int r = 0; r < TG_RW; ++r) tsne_quad<MODE, true>(n, row[r], j0, yix[r], yiy[r], xj, yj, p[r], e, zf, invz, a0[r], a1[r], kl[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < TG_RW; ++r) {
    const float s0 = wave_sum(a0[r]);
    const bool live = r0 + r < n && lane == 0;
    if (MODE == 0) {
      if (live) zrow[row[r]] = s0;
    } else {
      const float s1 = wave_sum(a1[r]);
      if (live) {
        grad[2 * row[r]] = 4.f * s0;
        grad[2 * row[r] + 1] = 4.f * s1;
      }
      if (MODE == 2) {
        const double k = wave_sum_d(kl[r]);
        if (live) klrow[row[r]] = k;
      }
    }
  }
}

// scikit-learn's _gradient_descent body on the 2 n values of the state; record = {KL or NaN, |gains * grad|_2, Z, 0}
__global__ __launch_bounds__(SUM_THREADS) void k_tsne_update(int n, float* __restrict__ Y, float* __restrict__ U, float* __restrict__ G,
                                                             const float* __restrict__ grad, float momentum, float lr,
                                                             const double* __restrict__ klrow, const double* __restrict__ Zp,
                                                             int have_kl, double* __restrict__ record) {
  __shared__ double sh0[SUM_THREADS / WAVE], sh1[SUM_THREADS / WAVE];
  double gn = 0.0, kl = 0.0;
  for (int t = threadIdx.x; t < 2 * n; t += SUM_THREADS) {
    const float g = grad[t];
    float u = U[t], gain = G[t];
    gain = u * g < 0.f ? gain + 0.2f : gain * 0.8f;
    gain = fmaxf(gain, 0.01f);
    const float gg = g * gain;
    u = momentum * u - lr * gg;
    U[t] = u;
    G[t] = gain;
    Y[t] += u;
    gn += (double)gg * (double)gg;
  }
  if (have_kl)
    for (int t = threadIdx.x; t < n; t += SUM_THREADS) kl += klrow[t];
  gn = block_sum_d<SUM_THREADS / WAVE>(gn, sh0);
  kl = block_sum_d<SUM_THREADS / WAVE>(kl, sh1);
  if (threadIdx.x == 0) {
    record[0] = have_kl ? kl : (double)NAN;
    record[1] = sqrt(gn);
    record[2] = Zp[0];
    record[3] = 0.0;
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// workspace: Z (one double in 256 bytes) | zrow fp32 [n] | klrow / row totals fp64 [n]
struct TsnePlan {
  size_t o_z, o_zrow, o_rows, total;
};

static bool tsne_shape_ok(int n, int ld) {
  return n >= 2 && (long long)n * n < 2147483648ll && ld >= n && ld % 4 == 0 && ld - n < 4;
}

static void tsne_plan(int n, TsnePlan* p) {
  p->o_z = 0;
  p->o_zrow = 256;
  p->o_rows = p->o_zrow + ws_align((size_t)n * 4);
  p->total = p->o_rows + ws_align((size_t)n * 8) + 256;   // + 256: the base is aligned up inside the call
}

static inline int tsne_launched() { return hipGetLastError() == hipSuccess ? CGCN_OK : CGCN_ERR_LAUNCH; }

extern "C" {

size_t cgcn_tsne_workspace_bytes(int n) {
  if (!tsne_shape_ok(n, (n + 3) & ~3)) return 0;
  TsnePlan p;
  tsne_plan(n, &p);
  return p.total;
}

int cgcn_tsne_sqdist(cgcn_stream_t stream, int n, int d, int ld, const float* X, float* D) {
  if (!tsne_shape_ok(n, ld) || d < 4 || d % 4) return CGCN_ERR_UNSUPPORTED;
  if (!X || !D || ts_misaligned16(X)) return CGCN_ERR_BAD_ARG;
  const unsigned t = (unsigned)((n + SQ_T - 1) / SQ_T);
  hipLaunchKernelGGL(k_tsne_sqdist, dim3(t, t), dim3(256), 0, (hipStream_t)stream, n, d, ld, X, D);
  return tsne_launched();
}

int cgcn_tsne_affinities(cgcn_stream_t stream, int n, int ld, const float* D, float perplexity, float* C, double* beta) {
  if (!tsne_shape_ok(n, ld)) return CGCN_ERR_UNSUPPORTED;
  if (!D || !C || !beta || !(perplexity > 0.f)) return CGCN_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_tsne_affinities, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, n, ld, D, log((double)perplexity), C,
                     beta);
  return tsne_launched();
}

int cgcn_tsne_symmetrize(cgcn_stream_t stream, int n, int ld, const float* C, float* P, void* workspace, size_t workspace_bytes) {
  if (!tsne_shape_ok(n, ld)) return CGCN_ERR_UNSUPPORTED;
  if (!C || !P || !workspace) return CGCN_ERR_BAD_ARG;
  TsnePlan p;
  tsne_plan(n, &p);
  if (workspace_bytes < p.total) return CGCN_ERR_WORKSPACE;
  char* w = ws_base(workspace);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_tsne_rowsum, dim3((unsigned)n), dim3(256), 0, st, n, ld, C, (double*)(w + p.o_rows));
  hipLaunchKernelGGL(k_tsne_total<double>, dim3(1), dim3(SUM_THREADS), 0, st, n, (const double*)(w + p.o_rows), 2.0, (double*)(w + p.o_z));
  const unsigned t = (unsigned)((n + SQ_T - 1) / SQ_T);
  hipLaunchKernelGGL(k_tsne_symmetrize, dim3(t, t), dim3(256), 0, st, n, ld, C, P, (const double*)(w + p.o_z));
  return tsne_launched();
}

int cgcn_tsne_gradient(cgcn_stream_t stream, int n, int ld, const float* P, const float* Y, float exaggeration, float* grad,
                       int want_kl, void* workspace, size_t workspace_bytes) {
  if (!tsne_shape_ok(n, ld)) return CGCN_ERR_UNSUPPORTED;
  if (!P || !Y || !grad || !workspace || ts_misaligned16(P) || ((uintptr_t)Y & 7u)) return CGCN_ERR_BAD_ARG;
  TsnePlan p;
  tsne_plan(n, &p);
  if (workspace_bytes < p.total) return CGCN_ERR_WORKSPACE;
  char* w = ws_base(workspace);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((n + TG_ROWS - 1) / TG_ROWS)), block(TG_THREADS);
  double* Z = (double*)(w + p.o_z);
  float* zrow = (float*)(w + p.o_zrow);
  double* klrow = (double*)(w + p.o_rows);
  hipLaunchKernelGGL(k_tsne_pass<0>, grid, block, 0, st, n, ld, (const float*)nullptr, Y, 1.f, (const double*)nullptr, zrow,
                     (float*)nullptr, (double*)nullptr);
  hipLaunchKernelGGL(k_tsne_total<float>, dim3(1), dim3(SUM_THREADS), 0, st, n, (const float*)zrow, 1.0, Z);
  if (want_kl)
    hipLaunchKernelGGL(k_tsne_pass<2>, grid, block, 0, st, n, ld, P, Y, exaggeration, (const double*)Z, (float*)nullptr, grad, klrow);
  else
    hipLaunchKernelGGL(k_tsne_pass<1>, grid, block, 0, st, n, ld, P, Y, exaggeration, (const double*)Z, (float*)nullptr, grad,
                       (double*)nullptr);
  return tsne_launched();
}

int cgcn_tsne_update(cgcn_stream_t stream, int n, float* Y, float* update, float* gains, const float* grad, float momentum,
                     float learning_rate, int have_kl, double* record, void* workspace, size_t workspace_bytes) {
  if (!tsne_shape_ok(n, (n + 3) & ~3)) return CGCN_ERR_UNSUPPORTED;
  if (!Y || !update || !gains || !grad || !record || !workspace) return CGCN_ERR_BAD_ARG;
  TsnePlan p;
  tsne_plan(n, &p);
  if (workspace_bytes < p.total) return CGCN_ERR_WORKSPACE;
  char* w = ws_base(workspace);
  hipLaunchKernelGGL(k_tsne_update, dim3(1), dim3(SUM_THREADS), 0, (hipStream_t)stream, n, Y, update, gains, grad, momentum,
                     learning_rate, (const double*)(w + p.o_rows), (const double*)(w + p.o_z), have_kl, record);
  return tsne_launched();
}

}   // extern "C"
