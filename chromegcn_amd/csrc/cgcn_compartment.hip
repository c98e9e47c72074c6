// chromegcn_amd/csrc/cgcn_compartment.hip
//
// The dense middle of the A/B compartment call of one chromosome's contact matrix (DESIGN.md section 4.18;
// chromegcn_amd/compartments.py holds the rule and its numpy restatements): the balanced matrix over the kept bins, its sums
// per distance, the observed / expected map and its standardised rows, the Pearson map C = Z Z^T, and one step of the
// deflated power iteration on C.  Every dense operand is fp64, row-major, m rows (m <= 8192 kept bins); B / M / Z have a
// leading dimension ld >= m that is even, so that every row starts on 16 bytes; C is m x m.
//
//   k_comp_dense     a wavefront owns a bin of the CSR; its lanes stride over the row's entries and store
//                    val / (nv[a] nv[b]) at (rank[a], rank[b]) when both bins are kept.  Each stored entry is written once.
//   k_comp_dist      a wavefront owns a distance d: lane l adds B[i, rank[keep[i] + d]] over i = l, l + 64, ... ascending
//                    (a bin that is not kept adds nothing), one fixed butterfly, lane 0 stores dsum[d].
//   k_comp_oe_stats  a wavefront owns a row: pass 1 writes M in place and adds it up (lane l the columns l, l + 64, ...),
//                    mean = sum / m; pass 2 adds (M - mean)^2 in the same order.
//   k_comp_z         Z = (M - mean) / sqrt(ss) in place, one thread per element; a row with ss == 0 becomes 0.
//   k_comp_corr      a workgroup owns a 64 x 64 tile of C with tile column >= tile row: the two 64 x 16 operand tiles go
//                    through LDS (16-byte global loads; rows beyond m and columns beyond m are zeros there), each of the four
//                    wavefronts owns a 32 x 32 quadrant as 2 x 2 v_mfma_f64_16x16x4_f64 tiles, K ascending in one
//                    accumulator chain per element.  An element with column >= row is stored to (i, j) and to (j, i).
//   k_comp_matvec    a wavefront owns a row of C: y[i] = sum_j C[i, j] v[j], lanes striding, one fixed butterfly.
//   k_comp_finish    one workgroup: the dots with the earlier vectors, the deflation, lambda = v.y, |y|^2,
//                    |y - lambda v|^2 (per-thread partials in ascending order, a butterfly per wavefront, the wavefronts'
//                    sums added in order), v_next = y / |y|, and the record.
// No floating-point atomic, no split K, no order that scheduling could change: the same bits in every run.  The sums that the
// numpy restatement mirrors term by term (dist, mean, ss) use __dadd_rn / __dmul_rn so that nothing is contracted.  Nothing
// is allocated, nothing synchronises.
#include "cgcn_hicmap.hpp"

#define CMP_THREADS 256
#define CMP_WAVES (CMP_THREADS / WAVE)
#define CMP_MAX_BLOCKS 2048
#define CMP_MAX_M 8192
#define CMP_TILE 64
#define CMP_KT 16
#define CMP_LDS_LD (CMP_KT + 1)
#define CMP_FIN_THREADS 1024
#define CMP_MAX_PREV 2

typedef double cmp_d4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(CMP_THREADS) void k_comp_dense(int n, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                            const double* __restrict__ val, const double* __restrict__ norm,
                                                            long long n_norm, const int* __restrict__ rank, int m, int ld,
                                                            double* __restrict__ B) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long long waves = (long long)gridDim.x * CMP_WAVES;
  for (long long bin = (long long)blockIdx.x * CMP_WAVES + threadIdx.x / WAVE; bin < n; bin += waves) {
    const int ra = rank[bin];
    if (ra < 0 || ra >= m) continue;   // the whole wavefront
    const double na = norm ? hm_norm_at(norm, n_norm, bin) : 1.0;
    const int end = rowptr[bin + 1];
    for (int p = rowptr[bin] + lane; p < end; p += WAVE) {
      const int c = col[p];
      if (c < 0 || c >= n) continue;
      const int rc = rank[c];
      if (rc < 0 || rc >= m) continue;
      double v = val[p];
      if (norm) v = v / (na * hm_norm_at(norm, n_norm, c));   // one multiply, one divide
      B[(long long)ra * ld + rc] = v;
    }
  }
}

__global__ __launch_bounds__(CMP_THREADS) void k_comp_dist(int n, int m, int ld, const double* __restrict__ B,
                                                           const int* __restrict__ keep, const int* __restrict__ rank,
                                                           double* __restrict__ dsum) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long long waves = (long long)gridDim.x * CMP_WAVES;
  for (long long d = (long long)blockIdx.x * CMP_WAVES + threadIdx.x / WAVE; d < n; d += waves) {
    double acc = 0.0;
    for (int i = lane; i < m; i += WAVE) {
      const int kb = keep[i];
      if (kb < 0 || kb >= n) continue;
      const long long b = (long long)kb + d;
      if (b >= n) continue;
      const int r = rank[b];
      if (r < 0 || r >= m) continue;
      acc = __dadd_rn(acc, B[(long long)i * ld + r]);
    }
    acc = wave_sum_d(acc);
    if (lane == 0) dsum[d] = acc;
  }
}

__global__ __launch_bounds__(CMP_THREADS) void k_comp_oe_stats(int m, int ld, double* __restrict__ B, const int* __restrict__ keep,
                                                               const double* __restrict__ e, int n_e, int ignore_diags,
                                                               double* __restrict__ mean, double* __restrict__ ss) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long long waves = (long long)gridDim.x * CMP_WAVES;
  for (long long row = (long long)blockIdx.x * CMP_WAVES + threadIdx.x / WAVE; row < m; row += waves) {
    double* __restrict__ r = B + row * ld;
    const int ki = keep[row];
    double acc = 0.0;
    for (int j = lane; j < m; j += WAVE) {
      const long long dd = (long long)keep[j] - ki;
      const long long d = dd < 0 ? -dd : dd;
      const double ev = d < n_e ? e[d] : 0.0;
      const double v = (d >= ignore_diags && ev > 0.0) ? r[j] / ev : 1.0;
      r[j] = v;
      acc = __dadd_rn(acc, v);
    }
    const double mu = wave_sum_d(acc) / (double)m;
    acc = 0.0;
    for (int j = lane; j < m; j += WAVE) {   // a lane reads back what it wrote itself
      const double t = __dsub_rn(r[j], mu);
      acc = __dadd_rn(acc, __dmul_rn(t, t));
    }
    acc = wave_sum_d(acc);
    if (lane == 0) {
      mean[row] = mu;
      ss[row] = acc;
    }
  }
}

__global__ __launch_bounds__(CMP_THREADS) void k_comp_z(int m, int ld, double* __restrict__ B, const double* __restrict__ mean,
                                                        const double* __restrict__ ss) {
  const long long total = (long long)m * m;
  for (long long t = (long long)blockIdx.x * CMP_THREADS + threadIdx.x; t < total; t += (long long)gridDim.x * CMP_THREADS) {
    const int i = (int)(t / m), j = (int)(t % m);
    const double s = ss[i];
    double* p = B + (long long)i * ld + j;
    *p = s > 0.0 ? __dsub_rn(*p, mean[i]) / __dsqrt_rn(s) : 0.0;
  }
}

__global__ __launch_bounds__(CMP_THREADS) void k_comp_corr(int m, int ld, const double* __restrict__ Z, double* __restrict__ C) {
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (tj < ti) return;   // the whole workgroup: the lower tiles are the mirrored stores of the upper ones
  __shared__ double sA[CMP_TILE][CMP_LDS_LD], sB[CMP_TILE][CMP_LDS_LD];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;   // this wavefront's quadrant of the tile
  const int lr = lane & 15, lk = lane >> 4;                // A[row lr][k lk], B[k lk][col lr]: one f64 per lane
  cmp_d4 acc00 = {0.0, 0.0, 0.0, 0.0}, acc01 = acc00, acc10 = acc00, acc11 = acc00;
  for (int k0 = 0; k0 < m; k0 += CMP_KT) {
    for (int t = tid; t < CMP_TILE * (CMP_KT / 2); t += CMP_THREADS) {
      const int r = t / (CMP_KT / 2), c2 = (t % (CMP_KT / 2)) * 2;
      const int k = k0 + c2, ra = ti * CMP_TILE + r, rb = tj * CMP_TILE + r;
      double2 a = make_double2(0.0, 0.0), b = a;
      if (k < m) {   // k is even and ld is even and >= m: k + 1 < ld, the pair is inside the row
        if (ra < m) a = *reinterpret_cast<const double2*>(Z + (long long)ra * ld + k);
        if (rb < m) b = *reinterpret_cast<const double2*>(Z + (long long)rb * ld + k);
        if (k + 1 >= m) a.y = b.y = 0.0;
      }
      sA[r][c2] = a.x;
      sA[r][c2 + 1] = a.y;
      sB[r][c2] = b.x;
      sB[r][c2 + 1] = b.y;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < CMP_KT; kk += 4) {
      const double a0 = sA[wr + lr][kk + lk], a1 = sA[wr + 16 + lr][kk + lk];
      const double b0 = sB[wc + lr][kk + lk], b1 = sB[wc + 16 + lr][kk + lk];
      acc00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc00, 0, 0, 0);
      acc01 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc01, 0, 0, 0);
      acc10 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc10, 0, 0, 0);
      acc11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc11, 0, 0, 0);
    }
    __syncthreads();
  }
  // the f64 C/D layout: col = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const cmp_d4 acc = q == 0 ? acc00 : q == 1 ? acc01 : q == 2 ? acc10 : acc11;
    const int i0 = ti * CMP_TILE + wr + (q >> 1) * 16 + (lane >> 4), j = tj * CMP_TILE + wc + (q & 1) * 16 + (lane & 15);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int i = i0 + 4 * reg;
      if (i < m && j < m && j >= i) {
        C[(long long)i * m + j] = acc[reg];
        C[(long long)j * m + i] = acc[reg];
      }
    }
  }
}

__global__ __launch_bounds__(CMP_THREADS) void k_comp_matvec(int m, const double* __restrict__ C, const double* __restrict__ v,
                                                             double* __restrict__ y) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long long waves = (long long)gridDim.x * CMP_WAVES;
  for (long long row = (long long)blockIdx.x * CMP_WAVES + threadIdx.x / WAVE; row < m; row += waves) {
    const double* __restrict__ r = C + row * m;
    double acc = 0.0;
    for (int j = lane; j < m; j += WAVE) acc += r[j] * v[j];
    acc = wave_sum_d(acc);
    if (lane == 0) y[row] = acc;
  }
}

// The sum over the workgroup, the same value in every thread: a butterfly per wavefront, then the wavefronts in order.  Not
// block_sum_d: its barriers stand in front of the write and of the read, none behind the read, and without that one the
// compiler moves k_comp_finish's next loads up into the sum and takes two more registers.
__device__ __forceinline__ double cmp_block_sum(double v, double* s) {
  v = wave_sum_d(v);
  if ((threadIdx.x & (WAVE - 1)) == 0) s[threadIdx.x / WAVE] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < CMP_FIN_THREADS / WAVE; ++w) t += s[w];
  __syncthreads();
  return t;
}

__global__ __launch_bounds__(CMP_FIN_THREADS) void k_comp_finish(int m, const double* __restrict__ v, const double* __restrict__ prev,
                                                                 int n_prev, double* __restrict__ y, double* __restrict__ v_next,
                                                                 double* __restrict__ rec) {
  __shared__ double s[CMP_FIN_THREADS / WAVE];
  const int tid = threadIdx.x;
  double dot[CMP_MAX_PREV] = {0.0, 0.0};
#pragma unroll
  for (int p = 0; p < CMP_MAX_PREV; ++p) {
    if (p < n_prev) {   // the whole workgroup
      double acc = 0.0;
      for (int i = tid; i < m; i += CMP_FIN_THREADS) acc += prev[(long long)p * m + i] * y[i];
      dot[p] = cmp_block_sum(acc, s);
    }
  }
  double lam = 0.0, nn = 0.0;
  for (int i = tid; i < m; i += CMP_FIN_THREADS) {   // a thread owns its elements of y from here on
    double yi = y[i];
#pragma unroll
    for (int p = 0; p < CMP_MAX_PREV; ++p)
      if (p < n_prev) yi -= dot[p] * prev[(long long)p * m + i];
    y[i] = yi;
    lam += v[i] * yi;
    nn += yi * yi;
  }
  lam = cmp_block_sum(lam, s);
  nn = cmp_block_sum(nn, s);
  double r2 = 0.0;
  for (int i = tid; i < m; i += CMP_FIN_THREADS) {
    const double t = y[i] - lam * v[i];
    r2 += t * t;
  }
  r2 = cmp_block_sum(r2, s);
  const double len = __dsqrt_rn(nn);
  for (int i = tid; i < m; i += CMP_FIN_THREADS) v_next[i] = len > 0.0 ? y[i] / len : y[i];
  if (tid == 0) {
    rec[0] = lam;
    rec[1] = nn;
    rec[2] = r2;
    rec[3] = dot[0];
    rec[4] = dot[1];
  }
}

static inline unsigned cmp_wave_blocks(long long items) {
  long long blocks = (items + CMP_WAVES - 1) / CMP_WAVES;
  return (unsigned)(blocks > CMP_MAX_BLOCKS ? CMP_MAX_BLOCKS : blocks);
}

static inline int cmp_check_dense(int m, int ld, const void* B) {
  if (m < 0 || ld < m || (ld & 1) || (m > 0 && (!B || ((uintptr_t)B & 15)))) return CGCN_ERR_BAD_ARG;
  return m > CMP_MAX_M ? CGCN_ERR_UNSUPPORTED : CGCN_OK;
}

extern "C" {

int cgcn_hiccomp_dense(cgcn_stream_t stream, int n, const int32_t* rowptr, const int32_t* col, const double* val,
                       const double* norm, long long n_norm, const int32_t* rank, int m, int ld, double* B) {
  if (n < 0 || n_norm < 0 || (norm && n_norm < 1)) return CGCN_ERR_BAD_ARG;
  const int rc = cmp_check_dense(m, ld, B);
  if (rc != CGCN_OK) return rc;
  if (n == 0 || m == 0) return CGCN_OK;
  if (!rowptr || !col || !val || !rank) return CGCN_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_comp_dense, dim3(cmp_wave_blocks(n)), dim3(CMP_THREADS), 0, (hipStream_t)stream, n, rowptr, col, val, norm,
                     n_norm, rank, m, ld, B);
  return launch_status();
}

int cgcn_hiccomp_dist_sums(cgcn_stream_t stream, int n, int m, int ld, const double* B, const int32_t* keep, const int32_t* rank,
                           double* dsum) {
  if (n < 0) return CGCN_ERR_BAD_ARG;
  const int rc = cmp_check_dense(m, ld, B);
  if (rc != CGCN_OK) return rc;
  if (n == 0) return CGCN_OK;
  if (!dsum || !rank || (m > 0 && !keep)) return CGCN_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_comp_dist, dim3(cmp_wave_blocks(n)), dim3(CMP_THREADS), 0, (hipStream_t)stream, n, m, ld, B, keep, rank, dsum);
  return launch_status();
}

int cgcn_hiccomp_oe_rows(cgcn_stream_t stream, int m, int ld, double* B, const int32_t* keep, const double* e, int n_e,
                         int ignore_diags, int stages, double* mean, double* ss) {
  if (n_e < 0 || ignore_diags < 0 || stages < 1 || stages > 3) return CGCN_ERR_BAD_ARG;
  const int rc = cmp_check_dense(m, ld, B);
  if (rc != CGCN_OK) return rc;
  if (m == 0) return CGCN_OK;
  if (!mean || !ss || ((stages & 1) && (!keep || (n_e > 0 && !e)))) return CGCN_ERR_BAD_ARG;
  if (stages & 1) {
    hipLaunchKernelGGL(k_comp_oe_stats, dim3(cmp_wave_blocks(m)), dim3(CMP_THREADS), 0, (hipStream_t)stream, m, ld, B, keep, e, n_e,
                       ignore_diags, mean, ss);
    if (launch_status() != CGCN_OK) return CGCN_ERR_LAUNCH;
  }
  if (stages & 2) {
    long long blocks = ((long long)m * m + CMP_THREADS - 1) / CMP_THREADS;
    if (blocks > CMP_MAX_BLOCKS) blocks = CMP_MAX_BLOCKS;
    hipLaunchKernelGGL(k_comp_z, dim3((unsigned)blocks), dim3(CMP_THREADS), 0, (hipStream_t)stream, m, ld, B, mean, ss);
  }
  return launch_status();
}

int cgcn_hiccomp_corr(cgcn_stream_t stream, int m, int ld, const double* Z, double* C) {
  const int rc = cmp_check_dense(m, ld, Z);
  if (rc != CGCN_OK) return rc;
  if (m == 0) return CGCN_OK;
  if (!C) return CGCN_ERR_BAD_ARG;
  const unsigned tiles = (unsigned)((m + CMP_TILE - 1) / CMP_TILE);
  hipLaunchKernelGGL(k_comp_corr, dim3(tiles, tiles), dim3(CMP_THREADS), 0, (hipStream_t)stream, m, ld, Z, C);
  return launch_status();
}

int cgcn_hiccomp_step(cgcn_stream_t stream, int m, const double* C, const double* v, const double* prev, int n_prev, double* y,
                      double* v_next, double* rec) {
  if (m < 1 || n_prev < 0 || !C || !v || !y || !v_next || !rec || (n_prev > 0 && !prev) || v_next == v) return CGCN_ERR_BAD_ARG;
  if (m > CMP_MAX_M || n_prev > CMP_MAX_PREV) return CGCN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_comp_matvec, dim3(cmp_wave_blocks(m)), dim3(CMP_THREADS), 0, (hipStream_t)stream, m, C, v, y);
  if (launch_status() != CGCN_OK) return CGCN_ERR_LAUNCH;
  hipLaunchKernelGGL(k_comp_finish, dim3(1), dim3(CMP_FIN_THREADS), 0, (hipStream_t)stream, m, v, prev, n_prev, y, v_next, rec);
  return launch_status();
}

}  // extern "C"
