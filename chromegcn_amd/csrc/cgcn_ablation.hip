// chromegcn_amd/csrc/cgcn_ablation.hip
//
// Label-pair Hi-C edge ablation (scripts/visualize.py:79-119, the TF-TF interaction map) on the sparsity pattern.
// For labels (i, j) with positive windows P_i, P_j: every stored entry (u, v) with u in P_i and v in P_j is removed from
// A-hat, the rows renormalised, the model run on both strands, and
//     M[i, j] = (base_i - abl_ij) / base_i,   base_i / abl_ij = mean over P_i of sigmoid(strand mean of logit i)
// on the full / ablated graph.  Two routes (chromegcn_amd/ablation.py):
//   restricted (L <= 2): only the rows of P_i change in any layer, so every (j, u in P_i) "instance" is recomputed from
//       the unablated forward's layer inputs:
//         k_abl_layer  masked aggregation of the kept neighbours (plain form: the kept entries only, so a row that keeps
//                      one of many neighbours has no cancellation; a row that keeps nothing is exactly zero, decided by
//                      the kept count; the renormalisation is decided by the kept SUM, which stored zeros leave 0),
//                      then U = H W + b, tanh, gate and residual mix for the 2 x 16 rows of one (u, 16 column labels)
//                      block in fp32 vector FMAs.  Layer 2 reads a neighbour's ablated layer-1
//                      value wherever it lies in P_i (and the row's own, as its residual input).
//         k_abl_head   label i's head on those rows (ReLU, eval BatchNorm, one dot product per strand, strand mean,
//                      sigmoid), a fixed-order mean over P_i, and M[i, j]
//   composed (any L): k_abl_mask writes the masked values and row scales on the unchanged pattern, the library's eval
//       forward runs over it, k_abl_reduce forms abl_ij and M[i, j].
// Set-up once per call: k_abl_bits (per-row label bitmask: the "v in P_j" test) and k_abl_lists (every label's positive
// rows in ascending order, and each row's rank in them).  Every sum is in a fixed order: results are bit-identical from
// call to call (the only atomics count removed entries, in integers).
#include "cgcn_common.hpp"

#define ABL_NT 256   // threads of every ablation kernel
#define ABL_JB 16    // column labels per workgroup of k_abl_layer
#define ABL_S 2      // strands: the ablation always runs both (visualize.py:110-112)

__device__ __forceinline__ bool abl_bit(const uint32_t* __restrict__ bits, int Wd, int row, int label) {
  return (bits[(size_t)row * Wd + (label >> 5)] >> (label & 31)) & 1u;
}

// bits[u * Wd + w] bit b  <=>  targets[u, 32 w + b] != 0
__global__ __launch_bounds__(ABL_NT) void k_abl_bits(int n, int C, int Wd, const float* __restrict__ targets,
                                                     uint32_t* __restrict__ bits) {
  const long long i = (long long)blockIdx.x * ABL_NT + threadIdx.x;
  if (i >= (long long)n * Wd) return;
  const int u = (int)(i / Wd), w = (int)(i % Wd);
  uint32_t m = 0;
  for (int b = 0; b < 32; ++b) {
    const int c = w * 32 + b;
    if (c < C && targets[(size_t)u * C + c] != 0.f) m |= 1u << b;
  }
  bits[i] = m;
}

// one workgroup per label c: lists[c * n + k] = k-th positive row (ascending), ranks[c * n + u] = k or -1, counts[c]
__global__ __launch_bounds__(ABL_NT) void k_abl_lists(int n, int Wd, const uint32_t* __restrict__ bits,
                                                      int* __restrict__ lists, int* __restrict__ ranks,
                                                      int* __restrict__ counts) {
  __shared__ int wave_tot[ABL_NT / WAVE];
  const int c = blockIdx.x, t = threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE;
  int* list = lists + (size_t)c * n;
  int* rank = ranks + (size_t)c * n;
  int run = 0;
  for (int base = 0; base < n; base += ABL_NT) {
    const int u = base + t;
    const bool pos = u < n && abl_bit(bits, Wd, u, c);
    const unsigned long long m = __ballot(pos);
    const int below = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_tot[wv] = __popcll(m);
    __syncthreads();
    int off = run;
    for (int w = 0; w < wv; ++w) off += wave_tot[w];
    int tot = 0;
    for (int w = 0; w < ABL_NT / WAVE; ++w) tot += wave_tot[w];
    if (u < n) rank[u] = pos ? off + below : -1;
    if (pos) list[off + below] = u;
    run += tot;
    __syncthreads();
  }
  if (t == 0) counts[c] = run;
}

// One gated layer for the instances (jb0 + jb, k), jb < ABL_JB, of row u = pos_list[k] (a row of P_i):
//   H = rs' * sum over kept entries (u, v) of val_uv * X_v,  kept <=> v not in P_j  (j = cols[jb0 + jb]),
//   rs' = row_scale[u] (1 if NULL) when nothing was removed, else 1 / (sum of the kept values); where that sum is 0 (stored
//   zeros, or values that cancel) the reference's `s == 0 -> 1` leaves row_scale[u]; a row that keeps nothing is exactly 0;
//   U = H W + b;  Z = tanh U;  g = sigmoid(Z . wg + cg);  X' = (1 - g) X_u + g Z.
// X_v is X[s, v] (the unablated layer input) unless X_inst is given and v is in P_i: then the instance's own ablated
// value X_inst[jb0 + jb, rank(v)].  Instance rows are [n_cols][n_pos][S][D].
template <int D>
__global__ __launch_bounds__(ABL_NT) void k_abl_layer(int n, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                      const float* __restrict__ val, const float* __restrict__ row_scale,
                                                      const float* __restrict__ X, const float* __restrict__ X_inst,
                                                      const float* __restrict__ W, const float* __restrict__ b,
                                                      const float* __restrict__ wg, const float* __restrict__ cg,
                                                      const uint32_t* __restrict__ bits, int Wd,
                                                      const int* __restrict__ pos_list, const int* __restrict__ pos_rank,
                                                      int n_pos, const int* __restrict__ cols, int n_cols,
                                                      float* __restrict__ X_out, int* __restrict__ removed) {
  constexpr int SD = ABL_S * D;
  constexpr int EPT = SD / ABL_NT;        // elements of an instance's [S][D] row per thread (1 or 2)
  constexpr int R = ABL_JB * ABL_S;       // rows of the dense step
  constexpr int GROUPS = ABL_NT / D;      // thread groups of the dense step (one column per thread in a group)
  constexpr int RPT = R / GROUPS;         // dense-step rows per thread
  __shared__ __attribute__((aligned(16))) float hs[R * D];
  __shared__ float gate_s[R];
  const int t = threadIdx.x, k = blockIdx.x, jb0 = blockIdx.y * ABL_JB;
  const int u = pos_list[k];
  const int e0 = t * EPT, s = e0 / D, c0 = e0 % D;
  int jl[ABL_JB];
#pragma unroll
  for (int jb = 0; jb < ABL_JB; ++jb) jl[jb] = jb0 + jb < n_cols ? cols[jb0 + jb] : -1;   // -1: padding, never stored

  // ---- masked aggregation (plain form: kept entries only, in CSR order)
  float acc[ABL_JB][EPT], wsum[ABL_JB];
  int kept[ABL_JB], rem[ABL_JB];
#pragma unroll
  for (int jb = 0; jb < ABL_JB; ++jb) {
    wsum[jb] = 0.f;
    kept[jb] = rem[jb] = 0;
#pragma unroll
    for (int q = 0; q < EPT; ++q) acc[jb][q] = 0.f;
  }
  const int p1 = rowptr[u + 1];
  for (int p = rowptr[u]; p < p1; ++p) {
    const int v = col[p];
    const float w = val ? val[p] : 1.f;
    const int rv = X_inst ? pos_rank[v] : -1;
    float xv[EPT];
    if (rv < 0) {
#pragma unroll
      for (int q = 0; q < EPT; ++q) xv[q] = X[((size_t)s * n + v) * D + c0 + q];
    }
#pragma unroll
    for (int jb = 0; jb < ABL_JB; ++jb) {
      const int j = jl[jb];
      if (j < 0) continue;
      if (abl_bit(bits, Wd, v, j)) { ++rem[jb]; continue; }
      wsum[jb] += w;
      ++kept[jb];
#pragma unroll
      for (int q = 0; q < EPT; ++q) {
        const float x = rv < 0 ? xv[q] : X_inst[((size_t)(jb0 + jb) * n_pos + rv) * SD + e0 + q];
        acc[jb][q] = fmaf(w, x, acc[jb][q]);
      }
    }
  }
  const float rs_u = row_scale ? row_scale[u] : 1.f;
#pragma unroll
  for (int jb = 0; jb < ABL_JB; ++jb) {
    const float sc = rem[jb] == 0 || wsum[jb] == 0.f ? rs_u : 1.f / wsum[jb];   // kept sum 0: the reference's s == 0 -> 1
#pragma unroll
    for (int q = 0; q < EPT; ++q) hs[(jb * ABL_S + s) * D + c0 + q] = kept[jb] > 0 ? acc[jb][q] * sc : 0.f;
  }
  __syncthreads();

  // ---- U = H W + b, Z = tanh U  (thread: column c of rows g*RPT .. g*RPT + RPT - 1; a wave reads one H row at a time)
  const int c = t % D, g = t / D;
  float ua[RPT];
#pragma unroll
  for (int m = 0; m < RPT; ++m) ua[m] = 0.f;
  for (int kk = 0; kk < D; kk += 4) {
    const float w0 = W[(kk + 0) * D + c], w1 = W[(kk + 1) * D + c], w2 = W[(kk + 2) * D + c], w3 = W[(kk + 3) * D + c];
#pragma unroll
    for (int m = 0; m < RPT; ++m) {
      const f32x4 h = *reinterpret_cast<const f32x4*>(&hs[(g * RPT + m) * D + kk]);
      float a = ua[m];
      a = fmaf(h.x, w0, a);
      a = fmaf(h.y, w1, a);
      a = fmaf(h.z, w2, a);
      a = fmaf(h.w, w3, a);
      ua[m] = a;
    }
  }
  const float bc = b[c];
  __syncthreads();   // every thread is done reading H
#pragma unroll
  for (int m = 0; m < RPT; ++m) hs[(g * RPT + m) * D + c] = tanhf(ua[m] + bc);
  __syncthreads();

  // ---- gate per row: one wave per row at a time, fixed-order wave sum
  const int lane = t & (WAVE - 1), wv = t / WAVE;
  const float cgv = cg[0];
  for (int r = wv; r < R; r += ABL_NT / WAVE) {
    float part = 0.f;
#pragma unroll
    for (int cc = lane; cc < D; cc += WAVE) part = fmaf(hs[r * D + cc], wg[cc], part);
    const float tot = wave_sum(part);
    if (lane == 0) gate_s[r] = sigmoidf_(tot + cgv);
  }
  __syncthreads();

  // ---- residual mix, store
#pragma unroll
  for (int jb = 0; jb < ABL_JB; ++jb) {
    if (jl[jb] < 0) continue;
    const int r = jb * ABL_S + s;
    const float gr = gate_s[r];
    const size_t inst = ((size_t)(jb0 + jb) * n_pos + k) * SD + e0;
#pragma unroll
    for (int q = 0; q < EPT; ++q) {
      const float xin = X_inst ? X_inst[inst + q] : X[((size_t)s * n + u) * D + c0 + q];
      X_out[inst + q] = (1.f - gr) * xin + gr * hs[r * D + c0 + q];
    }
    if (removed && t == 0) removed[(size_t)(jb0 + jb) * n_pos + k] = rem[jb];
  }
}

// Label i's eval head on rows of P_i and the mean of sigmoid(strand-mean logit) over them, in a fixed order (wave w takes
// positions w, w + 4, ... in turn; the four wave sums are added in wave order).
//   label < 0 (base mode): workgroup c = label c on the unablated rows X[s, pos_lists[c][k]]; base[c] = mean (NaN if P_c
//       is empty).
//   label = i >= 0: workgroup jb = column label cols[jb] on the instance rows X_inst[jb][k]; M[i, cols[jb]] =
//       (base[i] - mean) / base[i], exactly 0 when the pair removed no stored entry (sum of removed[jb][k]).
template <int D>
__global__ __launch_bounds__(ABL_NT) void k_abl_head(int n, int C, const float* __restrict__ X,
                                                     const float* __restrict__ X_inst, const float* __restrict__ bn_w,
                                                     const float* __restrict__ bn_b, const float* __restrict__ run_mean,
                                                     const float* __restrict__ run_var, float eps,
                                                     const float* __restrict__ W_out, const float* __restrict__ b_out,
                                                     const int* __restrict__ pos_lists, const int* __restrict__ pos_counts,
                                                     int label, int n_pos, const int* __restrict__ cols,
                                                     const int* __restrict__ removed, float* __restrict__ base,
                                                     float* __restrict__ M) {
  constexpr int CPL = D / WAVE;   // columns per lane
  __shared__ float wave_p[ABL_NT / WAVE];
  __shared__ int wave_r[ABL_NT / WAVE];
  const bool base_mode = label < 0;
  const int t = threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE;
  const int i = base_mode ? (int)blockIdx.x : label;
  const int jb = base_mode ? 0 : (int)blockIdx.x;
  const int np = base_mode ? pos_counts[i] : n_pos;
  const int* list = pos_lists + (size_t)i * n;
  float mu[CPL], sc[CPL], sh[CPL], wo[CPL];
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    const int c = lane + q * WAVE;
    mu[q] = run_mean[c];
    sc[q] = rsqrtf(run_var[c] + eps) * bn_w[c];
    sh[q] = bn_b[c];
    wo[q] = W_out[(size_t)i * D + c];
  }
  const float bo = b_out[i];
  float psum = 0.f;
  int rsum = 0;
  for (int kk = wv; kk < np; kk += ABL_NT / WAVE) {
    float l[ABL_S];
#pragma unroll
    for (int s = 0; s < ABL_S; ++s) {
      const float* row = base_mode ? X + ((size_t)s * n + list[kk]) * D : X_inst + (((size_t)jb * n_pos + kk) * ABL_S + s) * D;
      float part = 0.f;
#pragma unroll
      for (int q = 0; q < CPL; ++q) {
        const float y = fmaxf(row[lane + q * WAVE], 0.f);
        part = fmaf((y - mu[q]) * sc[q] + sh[q], wo[q], part);
      }
      l[s] = wave_sum(part) + bo;
    }
    psum += sigmoidf_((l[0] + l[1]) * 0.5f);
    if (!base_mode) rsum += removed[(size_t)jb * n_pos + kk];
  }
  if (lane == 0) {
    wave_p[wv] = psum;
    wave_r[wv] = rsum;
  }
  __syncthreads();
  if (t == 0) {
    const float tot = (wave_p[0] + wave_p[1]) + (wave_p[2] + wave_p[3]);
    const int rtot = (wave_r[0] + wave_r[1]) + (wave_r[2] + wave_r[3]);
    const float mean = np > 0 ? tot / (float)np : __builtin_nanf("");
    if (base_mode) {
      base[i] = mean;
    } else {
      const float b0 = base[i];
      M[(size_t)i * C + cols[jb]] = rtot == 0 ? 0.f : (b0 - mean) / b0;
    }
  }
}

// Masked graph of the composed route on the unchanged pattern: val_out = val (1 if NULL) with the entries (u in P_i,
// v in P_j) zeroed; row_scale_out as k_abl_layer's rs'; removed[0] += number of zeroed entries (caller-zeroed).
__global__ __launch_bounds__(ABL_NT) void k_abl_mask(int n, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                     const float* __restrict__ val, const float* __restrict__ row_scale,
                                                     const uint32_t* __restrict__ bits, int Wd, int li, int lj,
                                                     float* __restrict__ val_out, float* __restrict__ rs_out,
                                                     int* __restrict__ removed) {
  __shared__ int blk_rem;
  if (threadIdx.x == 0) blk_rem = 0;
  __syncthreads();
  const int u = blockIdx.x * ABL_NT + threadIdx.x;
  if (u < n) {
    const bool in_i = abl_bit(bits, Wd, u, li);
    int rem = 0, kept = 0;
    float sum = 0.f;
    for (int p = rowptr[u]; p < rowptr[u + 1]; ++p) {
      const float w = val ? val[p] : 1.f;
      const bool drop = in_i && abl_bit(bits, Wd, col[p], lj);
      val_out[p] = drop ? 0.f : w;
      if (drop) {
        ++rem;
      } else {
        sum += w;
        ++kept;
      }
    }
    const float rs_u = row_scale ? row_scale[u] : 1.f;
    rs_out[u] = rem == 0 ? rs_u : (sum != 0.f ? 1.f / sum : (kept > 0 ? rs_u : 0.f));   // kept sum 0: s == 0 -> 1
    if (rem) atomicAdd(&blk_rem, rem);
  }
  __syncthreads();
  if (threadIdx.x == 0 && blk_rem) atomicAdd(removed, blk_rem);
}

// mean over P_i of sigmoid((logits[0, u, i] + logits[1, u, i]) / 2), each thread over positions t, t + 256, ..., then a
// fixed tree; base mode (label < 0) / pair mode as in k_abl_head, the removed count from removed[0]
__global__ __launch_bounds__(ABL_NT) void k_abl_reduce(int n, int C, const float* __restrict__ logits,
                                                       const int* __restrict__ pos_lists, const int* __restrict__ pos_counts,
                                                       int label, int col_label, const int* __restrict__ removed,
                                                       float* __restrict__ base, float* __restrict__ M) {
  __shared__ float part[ABL_NT];
  const bool base_mode = label < 0;
  const int t = threadIdx.x;
  const int i = base_mode ? (int)blockIdx.x : label;
  const int np = pos_counts[i];
  const int* list = pos_lists + (size_t)i * n;
  float acc = 0.f;
  for (int kk = t; kk < np; kk += ABL_NT) {
    const size_t u = (size_t)list[kk];
    acc += sigmoidf_((logits[u * C + i] + logits[((size_t)n + u) * C + i]) * 0.5f);
  }
  part[t] = acc;
  __syncthreads();
  for (int off = ABL_NT / 2; off > 0; off >>= 1) {
    if (t < off) part[t] += part[t + off];
    __syncthreads();
  }
  if (t == 0) {
    const float mean = np > 0 ? part[0] / (float)np : __builtin_nanf("");
    if (base_mode) {
      base[i] = mean;
    } else {
      const float b0 = base[i];
      M[(size_t)i * C + col_label] = removed[0] == 0 ? 0.f : (b0 - mean) / b0;
    }
  }
}

static inline size_t abl_align(size_t b) { return (b + 255) & ~(size_t)255; }
static inline bool abl_dim_ok(int S, int d) { return S == ABL_S && (d == 128 || d == 256); }

extern "C" {

size_t cgcn_ablation_workspace_bytes(int n_inst, int S, int d, int layers) {
  if (n_inst < 0 || layers < 1 || layers > 2 || !abl_dim_ok(S, d)) return 0;
  const size_t feat = abl_align((size_t)n_inst * S * d * sizeof(float));
  return (size_t)layers * feat + abl_align((size_t)n_inst * sizeof(int32_t));
}

int cgcn_ablation_prepare(cgcn_stream_t stream, int n, int C, const float* targets, uint32_t* label_bits, int32_t* pos_lists,
                          int32_t* pos_ranks, int32_t* pos_counts) {
  if (n < 0 || C < 1) return CGCN_ERR_BAD_ARG;
  if (!pos_counts || (n > 0 && (!targets || !label_bits || !pos_lists || !pos_ranks))) return CGCN_ERR_BAD_ARG;
  if ((long long)n * C >= (1ll << 31)) return CGCN_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int Wd = (C + 31) / 32;
  if (n > 0) {
    const long long words = (long long)n * Wd;
    hipLaunchKernelGGL(k_abl_bits, dim3((unsigned)((words + ABL_NT - 1) / ABL_NT)), dim3(ABL_NT), 0, st, n, C, Wd, targets,
                       label_bits);
  }
  hipLaunchKernelGGL(k_abl_lists, dim3(C), dim3(ABL_NT), 0, st, n, Wd, label_bits, pos_lists, pos_ranks, pos_counts);
  return launch_status();
}

int cgcn_ablation_layer(cgcn_stream_t stream, int n, int S, int d, const int32_t* rowptr, const int32_t* col, const float* val,
                        const float* row_scale, const float* X, const float* X_inst, const float* W, const float* b,
                        const float* wg, const float* cg, const uint32_t* label_bits, int C, const int32_t* pos_list,
                        const int32_t* pos_rank, int n_pos, const int32_t* cols, int n_cols, float* X_out,
                        int32_t* removed) {
  if (n < 0 || n_pos < 0 || n_cols < 0 || C < 1) return CGCN_ERR_BAD_ARG;
  if (!abl_dim_ok(S, d)) return CGCN_ERR_UNSUPPORTED;
  if (!rowptr || !col || !X || !W || !b || !wg || !cg || !label_bits || !pos_list || !cols || !X_out) return CGCN_ERR_BAD_ARG;
  if (X_inst && !pos_rank) return CGCN_ERR_BAD_ARG;
  if (n_pos > n || (n_cols + ABL_JB - 1) / ABL_JB > 65535) return CGCN_ERR_UNSUPPORTED;
  if (n_pos == 0 || n_cols == 0) return CGCN_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(n_pos, (n_cols + ABL_JB - 1) / ABL_JB);
  const int Wd = (C + 31) / 32;
  if (d == 128)
    hipLaunchKernelGGL(k_abl_layer<128>, grid, dim3(ABL_NT), 0, st, n, rowptr, col, val, row_scale, X, X_inst, W, b, wg, cg,
                       label_bits, Wd, pos_list, pos_rank, n_pos, cols, n_cols, X_out, removed);
  else
    hipLaunchKernelGGL(k_abl_layer<256>, grid, dim3(ABL_NT), 0, st, n, rowptr, col, val, row_scale, X, X_inst, W, b, wg, cg,
                       label_bits, Wd, pos_list, pos_rank, n_pos, cols, n_cols, X_out, removed);
  return launch_status();
}

int cgcn_ablation_head(cgcn_stream_t stream, int n, int S, int d, int C, const float* X, const float* X_inst,
                       const float* bn_w, const float* bn_b, const float* run_mean, const float* run_var, float eps,
                       const float* W_out, const float* b_out, const int32_t* pos_lists, const int32_t* pos_counts,
                       int label, int n_pos, const int32_t* cols, int n_cols, const int32_t* removed, float* base,
                       float* M) {
  if (n < 0 || C < 1 || n_pos < 0 || n_cols < 0 || label >= C) return CGCN_ERR_BAD_ARG;
  if (!abl_dim_ok(S, d)) return CGCN_ERR_UNSUPPORTED;
  if (!bn_w || !bn_b || !run_mean || !run_var || !W_out || !b_out || !pos_lists || !base) return CGCN_ERR_BAD_ARG;
  const bool base_mode = label < 0;
  if (base_mode ? (!X || !pos_counts) : (!X_inst || !cols || !removed || !M)) return CGCN_ERR_BAD_ARG;
  if (!base_mode && n_pos > n) return CGCN_ERR_UNSUPPORTED;
  const int blocks = base_mode ? C : n_cols;
  if (blocks == 0) return CGCN_OK;
  hipStream_t st = (hipStream_t)stream;
  if (d == 128)
    hipLaunchKernelGGL(k_abl_head<128>, dim3(blocks), dim3(ABL_NT), 0, st, n, C, X, X_inst, bn_w, bn_b, run_mean, run_var, eps,
                       W_out, b_out, pos_lists, pos_counts, label, n_pos, cols, removed, base, M);
  else
    hipLaunchKernelGGL(k_abl_head<256>, dim3(blocks), dim3(ABL_NT), 0, st, n, C, X, X_inst, bn_w, bn_b, run_mean, run_var, eps,
                       W_out, b_out, pos_lists, pos_counts, label, n_pos, cols, removed, base, M);
  return launch_status();
}

int cgcn_ablation_mask(cgcn_stream_t stream, int n, int C, const int32_t* rowptr, const int32_t* col, const float* val,
                       const float* row_scale, const uint32_t* label_bits, int label_i, int label_j, float* val_out,
                       float* row_scale_out, int32_t* removed) {
  if (n < 0 || C < 1 || label_i < 0 || label_i >= C || label_j < 0 || label_j >= C) return CGCN_ERR_BAD_ARG;
  if (!removed || (n > 0 && (!rowptr || !col || !label_bits || !val_out || !row_scale_out))) return CGCN_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(removed, 0, sizeof(int32_t), st) != hipSuccess) return CGCN_ERR_LAUNCH;
  if (n > 0)
    hipLaunchKernelGGL(k_abl_mask, dim3((n + ABL_NT - 1) / ABL_NT), dim3(ABL_NT), 0, st, n, rowptr, col, val, row_scale,
                       label_bits, (C + 31) / 32, label_i, label_j, val_out, row_scale_out, removed);
  return launch_status();
}

int cgcn_ablation_reduce(cgcn_stream_t stream, int n, int S, int C, const float* logits, const int32_t* pos_lists,
                         const int32_t* pos_counts, int label, int col_label, const int32_t* removed, float* base, float* M) {
  if (n < 0 || C < 1 || label >= C || (label >= 0 && (col_label < 0 || col_label >= C))) return CGCN_ERR_BAD_ARG;
  if (S != ABL_S) return CGCN_ERR_UNSUPPORTED;
  if (!logits || !pos_lists || !pos_counts || !base || (label >= 0 && (!removed || !M))) return CGCN_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_abl_reduce, dim3(label < 0 ? C : 1), dim3(ABL_NT), 0, st, n, C, logits, pos_lists, pos_counts, label,
                     col_label, removed, base, M);
  return launch_status();
}

}  // extern "C"
