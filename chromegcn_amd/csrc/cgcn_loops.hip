// chromegcn_amd/csrc/cgcn_loops.hip
//
// Chromatin loops after HiCCUPS: pixels of one chromosome's contact matrix that are enriched over four LOCAL backgrounds
// (chromegcn_amd/loops.py holds the rule and its numpy restatement).
//
//   k_loops_band     CSR -> the dense raw band, band[i width + d] = A[i, i + d].  A wavefront owns row i: it finds the first
//                    column >= i by binary search and its lanes scatter the entries up to column i + width - 1 into the row,
//                    which the caller has zero-filled.  Each element is written at most once.
//   k_loops_pass1    a workgroup owns a tile of 8 rows x 32 distances in (i, d) coordinates.  It stages the balanced values, the
//                    participation bytes and the expected values of the skewed halo (w rows and 2 w distances either side) in
//                    LDS; a thread then runs its pixel's four sums over the (2 w + 1)^2 box ONCE, row-major, adding a cell to
//                    every neighbourhood that holds it: that is each neighbourhood's own listed order.  Candidate test, local
//                    expected values, chunk indices by comparison against the uploaded table, the packed record of the pixel,
//                    and the histogram: counts < 8 are collected in LDS (a wavefront's lanes that agree with its first lane on
//                    (chunk, count) go in as one add) and reach memory as one integer atomic per touched cell and tile.
//   k_loops_count / k_loops_write
//                    the ordered count / scan / write of the enriched pixels over the packed records (cgcn_compact.hpp), 256
//                    consecutive pixels of the (i, d) order per workgroup.  The writer repeats the sums of ITS pixels alone,
//                    reading the band directly: the same cells, operations and order as pass 1, hence the same bits.
// Every floating-point sum is sequential in a fixed order and the only atomics are integer ones: the same bits in every run.
// An fp64 division is IEEE here; contraction is off, so that no sum is fused with a product.
#include "cgcn_compact.hpp"
#include "cgcn_hicmap.hpp"

#pragma clang fp contract(off)

#define LP_THREADS 256
#define LP_TI 8                               // rows of a tile
#define LP_TD 32                              // distances of a tile: a 32-lane half reads one 256-byte bank row
#define LP_WMAX 10
#define LP_ROWS (LP_TI + 2 * LP_WMAX)         // 28
#define LP_COLS (LP_TD + 4 * LP_WMAX)         // 72
#define LP_BINS (LP_ROWS + LP_COLS)           // the column bins of a tile: fewer than rows + distances
#define LP_MAX_CHUNKS 64
#define LP_SMALL 8                            // counts below it are collected in LDS
#define LP_MAX_PIXELS (1ll << 28)

struct LpRule {
  int p, w, ignore_diags, min_dist;
  int full[4];   // the full sizes of donut, lower-left, horizontal, vertical
};

struct LpAcc {
  double sd, sl, sh, sv, td, tl, th, tv;
  int cd, cl, ch, cv;
};

// rule 2's validity of bin b and its norm value (1.0 without a vector); b may lie outside [0, n)
__device__ __forceinline__ bool lp_bin(const double* __restrict__ vc, const double* __restrict__ norm, long long n_norm, int n,
                                       long long b, double& nv) {
  nv = 1.0;
  if (b < 0 || b >= n) return false;
  return hm_bin(vc, norm, n_norm, b, nv);
}

// The four sums of one pixel.  cell(da, db, B, E, part): the balanced value (0 where the cell takes no part), the expected
// value of its distance and whether it takes part.  The branches depend on (da, db, p, w) alone: they are uniform.
template <class Cell>
__device__ __forceinline__ LpAcc lp_sums(const Cell& cell, int p, int w) {
  LpAcc a = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0};
  for (int da = -w; da <= w; ++da) {
    const int ada = da < 0 ? -da : da;
    for (int db = -w; db <= w; ++db) {
      const int adb = db < 0 ? -db : db;
      if (ada <= p && adb <= p) continue;
      double B, E;
      bool part;
      cell(da, db, B, E, part);
      const double e = part ? E : 0.0;
      const int c = part ? 1 : 0;
      if (da != 0 && db != 0) {
        a.sd += B, a.td += e, a.cd += c;
        if (da >= 1 && db <= -1) a.sl += B, a.tl += e, a.cl += c;
      }
      if (ada <= 1 && adb > p) a.sh += B, a.th += e, a.ch += c;
      if (adb <= 1 && ada > p) a.sv += B, a.tv += e, a.cv += c;
    }
  }
  return a;
}

__device__ __forceinline__ bool lp_enough(const LpAcc& a, const LpRule& r) {
  return a.td > 0.0 && a.tl > 0.0 && a.th > 0.0 && a.tv > 0.0 && 2 * a.cd >= r.full[0] && 2 * a.cl >= r.full[1] &&
         2 * a.ch >= r.full[2] && 2 * a.cv >= r.full[3];
}

// rule 6, in exactly this order
__device__ __forceinline__ double lp_lambda(double S, double T, double ex_d, double nvij) { return ((S / T) * ex_d) * nvij; }

// the number of boundaries <= lam; a NaN counts them all, as np.searchsorted(t, lam, 'right') does
__device__ __forceinline__ int lp_chunk(const double* t, int nb, double lam) {
  int lo = 0, hi = nb;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (!(lam < t[mid])) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int lp_count_of(double a, int W) {
  const double o = __builtin_rint(a);
  return o < (double)(W - 1) ? (int)o : W - 1;
}

__global__ __launch_bounds__(LP_THREADS) void k_loops_band(int n, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                           const double* __restrict__ val, int width, double* __restrict__ band) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long long waves = (long long)gridDim.x * (LP_THREADS / WAVE);
  for (long long row = (long long)blockIdx.x * (LP_THREADS / WAVE) + threadIdx.x / WAVE; row < n; row += waves) {
    const int i = (int)row, end = rowptr[i + 1];
    const int s = hm_row_lower(col, rowptr[i], end, i);   // the first entry of row i with a column >= i
    for (int q = s + lane; q < end; q += WAVE) {
      const long long d = (long long)col[q] - i;
      if (d >= width || col[q] >= n) break;   // the columns ascend: every later entry of this lane is outside too
      band[row * width + d] = val[q];
    }
  }
}

struct LpCellLds {
  const double* Bs;
  const unsigned char* Ps;
  const double* Es;
  int base, c0, lc;   // the pixel's own cell, its column and the row stride
  __device__ __forceinline__ void operator()(int da, int db, double& B, double& E, bool& part) const {
    const int dc = db - da, at = base + da * lc + dc;
    B = Bs[at];
    part = Ps[at] != 0;
    E = Es[c0 + dc];
  }
};

__global__ __launch_bounds__(LP_THREADS) void k_loops_pass1(int n, int D, int width, int tiles_d, const double* __restrict__ band,
                                                            const double* __restrict__ vc, const double* __restrict__ norm,
                                                            long long n_norm, const double* __restrict__ ex, long long n_ex,
                                                            LpRule rule, const double* __restrict__ bounds, int n_chunks, int W,
                                                            int* __restrict__ hist, uint32_t* __restrict__ flags,
                                                            double* __restrict__ lambda_out) {
  __shared__ double Bs[LP_ROWS * LP_COLS];
  __shared__ double Es[LP_COLS];
  __shared__ double nva[LP_ROWS], nvb[LP_BINS];
  __shared__ double tb[LP_MAX_CHUNKS];
  __shared__ int lh[4 * LP_MAX_CHUNKS * LP_SMALL];
  __shared__ unsigned char Ps[LP_ROWS * LP_COLS];
  __shared__ unsigned char oka[LP_ROWS], okb[LP_BINS];
  const int tid = threadIdx.x, w = rule.w, p = rule.p;
  const int i0 = (int)(blockIdx.x / tiles_d) * LP_TI, d0 = (int)(blockIdx.x % tiles_d) * LP_TD;
  const int rows = LP_TI + 2 * w, lc = LP_TD + 4 * w;
  const long long a0 = (long long)i0 - w, dd0 = (long long)d0 - 2 * w, b0 = a0 + dd0;
  for (int t = tid; t < rows; t += LP_THREADS) {
    double nv;
    oka[t] = lp_bin(vc, norm, n_norm, n, a0 + t, nv) ? 1 : 0;
    nva[t] = nv;
  }
  for (int t = tid; t < rows + lc; t += LP_THREADS) {
    double nv;
    okb[t] = lp_bin(vc, norm, n_norm, n, b0 + t, nv) ? 1 : 0;
    nvb[t] = nv;
  }
  for (int t = tid; t < lc; t += LP_THREADS) {
    const long long dd = dd0 + t;
    Es[t] = (dd >= 0 && dd < n_ex) ? ex[dd] : 0.0;
  }
  for (int t = tid; t < n_chunks - 1; t += LP_THREADS) tb[t] = bounds[t];
  for (int t = tid; t < 4 * LP_MAX_CHUNKS * LP_SMALL; t += LP_THREADS) lh[t] = 0;
  __syncthreads();
  for (int t = tid; t < rows * lc; t += LP_THREADS) {
    const int r = t / lc, c = t - r * lc;
    const long long a = a0 + r, dd = dd0 + c;
    const bool part = oka[r] && okb[r + c] && dd >= rule.ignore_diags && dd < width;   // oka / okb: both bins inside and valid
    double B = 0.0;
    if (part) B = band[a * width + dd] / (nva[r] * nvb[r + c]);
    Bs[t] = B;
    Ps[t] = part ? 1 : 0;
  }
  __syncthreads();
  const int ti = tid / LP_TD, td = tid % LP_TD;
  const int i = i0 + ti, d = d0 + td;
  const bool active = i < n && d <= D;
  const int r = ti + w, c = td + 2 * w;
  const LpCellLds cell = {Bs, Ps, Es, r * lc + c, c, lc};
  const LpAcc acc = lp_sums(cell, p, w);
  const bool cand = active && oka[r] && okb[r + c] && d >= rule.min_dist && lp_enough(acc, rule);
  const double nan = hm_nan();
  double lam[4] = {nan, nan, nan, nan};
  int k[4] = {0, 0, 0, 0}, o = 0;
  if (cand) {
    const double nvij = nva[r] * nvb[r + c], exd = Es[c];
    lam[0] = lp_lambda(acc.sd, acc.td, exd, nvij);
    lam[1] = lp_lambda(acc.sl, acc.tl, exd, nvij);
    lam[2] = lp_lambda(acc.sh, acc.th, exd, nvij);
    lam[3] = lp_lambda(acc.sv, acc.tv, exd, nvij);
#pragma unroll
    for (int x = 0; x < 4; ++x) k[x] = lp_chunk(tb, n_chunks - 1, lam[x]);
    o = lp_count_of(band[(long long)i * width + d], W);
  }
  if (active) {
    const long long q = (long long)i * (D + 1) + d;
    flags[q] = cand ? (0x80000000u | (uint32_t)k[0] | ((uint32_t)k[1] << 6) | ((uint32_t)k[2] << 12) | ((uint32_t)k[3] << 18)) : 0u;
    if (lambda_out) {
      const long long plane = (long long)n * (D + 1);
#pragma unroll
      for (int x = 0; x < 4; ++x) lambda_out[x * plane + q] = lam[x];
    }
  }
  // the histogram; every lane of the workgroup comes through here
  const int lane = tid & (WAVE - 1);
  const bool small = cand && o < LP_SMALL;
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    const int key = k[x] * LP_SMALL + o;
    const u64 m = __ballot(small);
    if (m) {
      const int lead = __ffsll((unsigned long long)m) - 1;
      const int key0 = __shfl(key, lead);
      const u64 same = __ballot(small && key == key0);
      if (lane == lead) atomicAdd(&lh[x * LP_MAX_CHUNKS * LP_SMALL + key0], __popcll(same));
      if (small && key != key0) atomicAdd(&lh[x * LP_MAX_CHUNKS * LP_SMALL + key], 1);
    }
    if (cand && !small) atomicAdd(&hist[((long long)x * n_chunks + k[x]) * W + o], 1);
  }
  __syncthreads();
  for (int t = tid; t < 4 * LP_MAX_CHUNKS * LP_SMALL; t += LP_THREADS) {
    const int v = lh[t];
    if (v) {
      const int x = t / (LP_MAX_CHUNKS * LP_SMALL), kk = (t / LP_SMALL) % LP_MAX_CHUNKS, oo = t % LP_SMALL;
      atomicAdd(&hist[((long long)x * n_chunks + kk) * W + oo], v);   // kk < n_chunks and oo < W: only such cells were touched
    }
  }
}

// rule 10 on the packed record of pixel q
__device__ __forceinline__ bool lp_enriched(long long q, long long n_pix, int D, int width, const double* __restrict__ band,
                                            const uint32_t* __restrict__ flags, const int* __restrict__ thr, int n_chunks, int W) {
  if (q >= n_pix) return false;
  const uint32_t pk = flags[q];
  if (!(pk >> 31)) return false;
  const long long i = q / (D + 1), d = q - i * (D + 1);
  const int o = lp_count_of(band[i * width + d], W);
  bool hit = true;
#pragma unroll
  for (int x = 0; x < 4; ++x) hit = hit && o >= thr[x * n_chunks + (int)((pk >> (6 * x)) & 63u)];
  return hit;
}

__global__ __launch_bounds__(LP_THREADS) void k_loops_count(long long n_pix, int D, int width, const double* __restrict__ band,
                                                            const uint32_t* __restrict__ flags, const int* __restrict__ thr,
                                                            int n_chunks, int W, int* __restrict__ counts) {
  __shared__ int wave_tot[LP_THREADS / WAVE];
  const long long q = (long long)blockIdx.x * LP_THREADS + threadIdx.x;
  const WgFlags<LP_THREADS / WAVE> f(lp_enriched(q, n_pix, D, width, band, flags, thr, n_chunks, W), wave_tot);
  if (threadIdx.x == 0) counts[blockIdx.x] = f.count();
}

struct LpCellGlobal {
  const double* band;
  const double* vc;
  const double* norm;
  const double* ex;
  long long n_norm, n_ex;
  int n, width, ignore_diags;
  long long i, d;
  __device__ __forceinline__ void operator()(int da, int db, double& B, double& E, bool& part) const {
    const long long a = i + da, dd = d + db - da;
    double na, nb;
    part = lp_bin(vc, norm, n_norm, n, a, na);
    part = lp_bin(vc, norm, n_norm, n, a + dd, nb) && part && dd >= ignore_diags && dd < width;
    B = 0.0;
    if (part) B = band[a * width + dd] / (na * nb);
    E = (dd >= 0 && dd < n_ex) ? ex[dd] : 0.0;
  }
};

__global__ __launch_bounds__(LP_THREADS) void k_loops_write(long long n_pix, int n, int D, int width, const double* __restrict__ band,
                                                            const double* __restrict__ vc, const double* __restrict__ norm,
                                                            long long n_norm, const double* __restrict__ ex, long long n_ex,
                                                            LpRule rule, const uint32_t* __restrict__ flags,
                                                            const int* __restrict__ thr, int n_chunks, int W,
                                                            const long long* __restrict__ off, long long capacity,
                                                            int* __restrict__ pix_ij, double* __restrict__ pix_val) {
  __shared__ int wave_tot[LP_THREADS / WAVE];
  const long long q = (long long)blockIdx.x * LP_THREADS + threadIdx.x;
  const bool hit = lp_enriched(q, n_pix, D, width, band, flags, thr, n_chunks, W);
  const WgFlags<LP_THREADS / WAVE> f(hit, wave_tot);
  const long long at = f.before(off[blockIdx.x]);
  if (!hit || at >= capacity) return;
  const long long i = q / (D + 1), d = q - i * (D + 1);
  const LpCellGlobal cell = {band, vc, norm, ex, n_norm, n_ex, n, width, rule.ignore_diags, i, d};
  const LpAcc acc = lp_sums(cell, rule.p, rule.w);
  double ni, nj;
  lp_bin(vc, norm, n_norm, n, i, ni);
  lp_bin(vc, norm, n_norm, n, i + d, nj);
  const double nvij = ni * nj, exd = ex[d];
  pix_ij[2 * at] = (int)i;
  pix_ij[2 * at + 1] = (int)(i + d);
  pix_val[5 * at] = band[i * width + d];
  pix_val[5 * at + 1] = lp_lambda(acc.sd, acc.td, exd, nvij);
  pix_val[5 * at + 2] = lp_lambda(acc.sl, acc.tl, exd, nvij);
  pix_val[5 * at + 3] = lp_lambda(acc.sh, acc.th, exd, nvij);
  pix_val[5 * at + 4] = lp_lambda(acc.sv, acc.tv, exd, nvij);
}

// the sizes every pass shares; CGCN_OK, or the error
static int lp_check(int n, int D, int width, int p, int w, int ignore_diags, int min_dist, int n_chunks, int W, long long n_norm,
                    long long n_ex) {
  if (n < 0 || D < 0 || p < 0 || w < 1 || p >= w || ignore_diags < 0 || min_dist < 0 || n_chunks < 2 || W < 1 || n_norm < 0 ||
      n_ex < 0)
    return CGCN_ERR_BAD_ARG;
  if (w > LP_WMAX || n_chunks > LP_MAX_CHUNKS || W > 65536 || (long long)n * ((long long)D + 1) > LP_MAX_PIXELS)
    return CGCN_ERR_UNSUPPORTED;
  if ((long long)width < (long long)D + 2 * w + 1) return CGCN_ERR_BAD_ARG;
  if (n_ex < (n < D + 1 ? n : D + 1)) return CGCN_ERR_BAD_ARG;   // a pixel's own distance is read from the vector
  return CGCN_OK;
}

static LpRule lp_rule(int p, int w, int ignore_diags, int min_dist) {
  LpRule r = {p, w, ignore_diags, min_dist, {0, 0, 0, 0}};
  r.full[0] = 4 * w * w - 4 * p * p;
  r.full[1] = w * w - p * p;
  r.full[2] = r.full[3] = 6 * (w - p);
  return r;
}

struct LpPlan {
  long long n_pix, nb;
  size_t counts, off, total;
};

static LpPlan lp_plan(int n, int D) {
  LpPlan pl;
  pl.n_pix = (long long)n * ((long long)D + 1);
  pl.nb = tiles_of(pl.n_pix, LP_THREADS);
  WsBump b = {0};
  pl.counts = b.take((size_t)pl.nb * sizeof(int));
  pl.off = b.take((size_t)pl.nb * sizeof(long long));
  pl.total = b.o + 256;
  return pl;
}

extern "C" {

int cgcn_hicloops_band(cgcn_stream_t stream, int n, const int32_t* rowptr, const int32_t* col, const double* val, int width,
                       double* band) {
  if (n < 0 || width < 1 || !rowptr) return CGCN_ERR_BAD_ARG;
  if (n > 0 && (!col || !val || !band)) return CGCN_ERR_BAD_ARG;
  if (n == 0) return CGCN_OK;
  long long blocks = ((long long)n + LP_THREADS / WAVE - 1) / (LP_THREADS / WAVE);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(k_loops_band, dim3((unsigned)blocks), dim3(LP_THREADS), 0, (hipStream_t)stream, n, rowptr, col, val, width,
                     band);
  return launch_status();
}

int cgcn_hicloops_pass1(cgcn_stream_t stream, int n, int D, int width, const double* band, const double* vc, const double* norm,
                        long long n_norm, const double* expected, long long n_expected, int p, int w, int ignore_diags,
                        int min_dist, const double* bounds, int n_chunks, int W, int32_t* hist, uint32_t* flags,
                        double* lambda_out) {
  const int rc = lp_check(n, D, width, p, w, ignore_diags, min_dist, n_chunks, W, n_norm, n_expected);
  if (rc != CGCN_OK) return rc;
  if (!bounds || !hist || (norm && n_norm < 1)) return CGCN_ERR_BAD_ARG;
  if (n > 0 && (!band || !vc || !expected || !flags)) return CGCN_ERR_BAD_ARG;
  if (n == 0) return CGCN_OK;
  const long long tiles_d = tiles_of((long long)D + 1, LP_TD), tiles = tiles_of(n, LP_TI) * tiles_d;
  hipLaunchKernelGGL(k_loops_pass1, dim3((unsigned)tiles), dim3(LP_THREADS), 0, (hipStream_t)stream, n, D, width, (int)tiles_d,
                     band, vc, norm, n_norm, expected, n_expected, lp_rule(p, w, ignore_diags, min_dist), bounds, n_chunks, W,
                     hist, flags, lambda_out);
  return launch_status();
}

size_t cgcn_hicloops_workspace_bytes(int n, int D) {
  if (n < 0 || D < 0 || (long long)n * ((long long)D + 1) > LP_MAX_PIXELS) return 0;
  return lp_plan(n, D).total;
}

int cgcn_hicloops_count(cgcn_stream_t stream, int n, int D, int width, const double* band, const uint32_t* flags,
                        const int32_t* thr, int n_chunks, int W, void* workspace, size_t workspace_bytes, long long* total) {
  if (n < 0 || D < 0 || width < D + 1 || n_chunks < 2 || W < 1 || !workspace || !total || !thr) return CGCN_ERR_BAD_ARG;
  if (n_chunks > LP_MAX_CHUNKS || W > 65536 || (long long)n * ((long long)D + 1) > LP_MAX_PIXELS) return CGCN_ERR_UNSUPPORTED;
  if (n > 0 && (!band || !flags)) return CGCN_ERR_BAD_ARG;
  const LpPlan pl = lp_plan(n, D);
  if (workspace_bytes < pl.total) return CGCN_ERR_WORKSPACE;
  char* base = ws_base(workspace);
  int* counts = (int*)(base + pl.counts);
  long long* off = (long long*)(base + pl.off);
  hipLaunchKernelGGL(k_loops_count, dim3((unsigned)pl.nb), dim3(LP_THREADS), 0, (hipStream_t)stream, pl.n_pix, D, width, band,
                     flags, thr, n_chunks, W, counts);
  hipLaunchKernelGGL(k_tile_scan<>, dim3(1), dim3(1024), 0, (hipStream_t)stream, (int)pl.nb, counts, off, total, (int*)nullptr,
                     0ll);
  return launch_status();
}

int cgcn_hicloops_write(cgcn_stream_t stream, int n, int D, int width, const double* band, const double* vc, const double* norm,
                        long long n_norm, const double* expected, long long n_expected, int p, int w, int ignore_diags,
                        const uint32_t* flags, const int32_t* thr, int n_chunks, int W, long long capacity, void* workspace,
                        size_t workspace_bytes, int32_t* pix_ij, double* pix_val) {
  const int rc = lp_check(n, D, width, p, w, ignore_diags, 0, n_chunks, W, n_norm, n_expected);
  if (rc != CGCN_OK) return rc;
  if (capacity < 0 || !workspace || !thr || (norm && n_norm < 1)) return CGCN_ERR_BAD_ARG;
  if (n > 0 && (!band || !vc || !expected || !flags)) return CGCN_ERR_BAD_ARG;
  if (capacity > 0 && (!pix_ij || !pix_val)) return CGCN_ERR_BAD_ARG;
  const LpPlan pl = lp_plan(n, D);
  if (workspace_bytes < pl.total) return CGCN_ERR_WORKSPACE;
  if (n == 0 || capacity == 0) return CGCN_OK;
  char* base = ws_base(workspace);
  hipLaunchKernelGGL(k_loops_write, dim3((unsigned)pl.nb), dim3(LP_THREADS), 0, (hipStream_t)stream, pl.n_pix, n, D, width, band,
                     vc, norm, n_norm, expected, n_expected, lp_rule(p, w, ignore_diags, 0), flags, thr, n_chunks, W,
                     (const long long*)(base + pl.off), capacity, pix_ij, pix_val);
  return launch_status();
}

}  // extern "C"
