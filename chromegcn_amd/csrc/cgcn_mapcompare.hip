// chromegcn_amd/csrc/cgcn_mapcompare.hip
//
// Two Hi-C contact maps compared by the stratum-adjusted correlation coefficient (DESIGN.md section 4.22;
// chromegcn_amd/mapcompare.py holds the rule and its numpy restatement).
//
//   k_mapcmp_smooth  the raw band of cgcn_hicloops_band -> the box SUMS of rule 3, stratum-major: S[d ld + i] for the cell
//                    (i, i + d).  A workgroup owns a tile of 32 rows x 32 COLUMNS (c = i + d): in (row, column) coordinates the
//                    box of a cell reaches h either way, so the halo is 2 h per side (in (row, distance) coordinates it would
//                    be 4 h along the distance).  The tile's cell values V(p, q), its halo included, are staged in LDS with the
//                    norm applied on load; a cell below the main diagonal reads its mirror image, a cell outside the matrix
//                    is 0.  Then the row sums R[p][c] = sum_db V(p, c + db), one sequential sum per element, and from them
//                    S = sum_da R[i + da][c]: rule 3's two levels, 2 (2 h + 1) LDS reads per output where the direct box
//                    takes (2 h + 1)^2.  The outputs go back through LDS (V is dead by then) so that the 32 lanes of a half
//                    wavefront store one diagonal of the tile: consecutive i of one stratum.
//                    LDS: ((32 + 2 h)^2 + 32 (32 + 2 h) + 2 (32 + 2 h)) doubles, 61 056 bytes at h = 20, sized per launch.
//   k_mapcmp_sums    one wavefront per (stratum, chunk of 2048 rows): lane l adds the rows c0 + l, c0 + l + 64, ... in
//                    ascending order, a cell that takes no part adds nothing, then the xor butterfly (wave_sum_d).  Pass 1:
//                    the cells, sum x, sum y; pass 2, with the means that the fold of pass 1 left on the device:
//                    sum (x - mx)^2, sum (y - my)^2, sum (x - mx)(y - my).
//   k_mapcmp_fold    one thread per stratum adds its chunk partials in chunk order; after pass 1 it also writes the means.
// Every floating-point sum has a fixed order and there are no atomics: the same bits in every run.  Contraction is off:
// every product and every sum is rounded on its own; an fp64 division is IEEE here.
#include "cgcn_compact.hpp"
#include "cgcn_hicmap.hpp"

#pragma clang fp contract(off)

#define MC_HMAX 20
#define MC_T 32                       // rows and columns of a smoothing tile
#define MC_THREADS 256
#define MC_CHUNK 2048                 // rows of one wavefront's chunk of a stratum
#define MC_MAX_ELEMS (1ll << 28)
#define MC_STATS 7                    // rows of `stats`: sum x, sum y, mean x, mean y, sxx, syy, sxy

__global__ __launch_bounds__(MC_THREADS) void k_mapcmp_smooth(int n, int D, int h, int width, const double* __restrict__ band,
                                                              const double* __restrict__ norm, long long n_norm, int ld,
                                                              int tiles_c, double* __restrict__ S) {
  extern __shared__ __attribute__((aligned(16))) double mc_lds[];
  const int E = MC_T + 2 * h;               // rows, and columns, of the staged tile
  double* V = mc_lds;                       // [E][E]; later the outputs [MC_T][MC_T]
  double* R = V + E * E;                    // [E][MC_T]
  double* nvp = R + E * MC_T;               // [E] norm values of the rows
  double* nvq = nvp + E;                    // [E] ... of the columns
  const int tid = threadIdx.x;
  const int ti = blockIdx.x / tiles_c, tc = blockIdx.x - ti * tiles_c;
  const long long i0 = (long long)ti * MC_T, c0 = i0 + (long long)tc * MC_T;
  const long long p0 = i0 - h, q0 = c0 - h;
  for (int k = tid; k < 2 * E; k += MC_THREADS) {
    const long long b = k < E ? p0 + k : q0 + (k - E);
    nvp[k] = norm ? hm_norm_at(norm, n_norm, b) : 1.0;   // nvq follows nvp
  }
  __syncthreads();
  for (int k = tid; k < E * E; k += MC_THREADS) {
    const int pl = k / E, ql = k - pl * E;
    const long long p = p0 + pl, q = q0 + ql;
    double v = 0.0;
    if (p >= 0 && p < n && q >= 0 && q < n) {
      const long long lo = p < q ? p : q, e = p < q ? q - p : p - q;
      if (e < width) {
        v = band[lo * width + e];
        if (norm) v = v / (nvp[pl] * nvq[ql]);
      }
    }
    V[k] = v;
  }
  __syncthreads();
  const int taps = 2 * h + 1;
  for (int k = tid; k < E * MC_T; k += MC_THREADS) {
    const int pl = k / MC_T, cl = k - pl * MC_T;
    const double* row = V + pl * E + cl;    // V(p, c - h) is at column cl of the staged tile
    double s = 0.0;
    for (int t = 0; t < taps; ++t) s += row[t];
    R[k] = s;
  }
  __syncthreads();
  for (int k = tid; k < MC_T * MC_T; k += MC_THREADS) {
    const int il = k / MC_T, cl = k - il * MC_T;
    const double* colp = R + il * MC_T + cl;   // R[i - h] is at row il
    double s = 0.0;
    for (int t = 0; t < taps; ++t) s += colp[t * MC_T];
    V[k] = (c0 + cl < n) ? s : 0.0;            // zeros beyond the matrix
  }
  __syncthreads();
  // one diagonal of the tile per half wavefront: dd = c - i - (c0 - i0) = -31 .. 31, lane = the row within the tile
  const int lane = tid & (MC_T - 1), grp = tid / MC_T;
  const long long dbase = c0 - i0;
  for (int g = grp; g < 2 * MC_T - 1; g += MC_THREADS / MC_T) {
    const int dd = g - (MC_T - 1);
    const long long d = dbase + dd, i = i0 + lane;
    const int cl = lane + dd;
    if (cl >= 0 && cl < MC_T && d >= 0 && d <= D && i < ld) S[d * ld + i] = V[lane * MC_T + cl];
  }
}

__global__ __launch_bounds__(MC_THREADS) void k_mapcmp_sums(int n, int D, int ld, const double* __restrict__ Sa,
                                                            const double* __restrict__ Sb, const uint8_t* __restrict__ valid,
                                                            int min_dist, int pass_no, int n_chunks,
                                                            const double* __restrict__ stats, double* __restrict__ part,
                                                            int* __restrict__ part_n) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long long w = (long long)blockIdx.x * (MC_THREADS / WAVE) + threadIdx.x / WAVE;
  if (w >= ((long long)D + 1) * n_chunks) return;
  const int d = (int)(w / n_chunks), ch = (int)(w - (long long)d * n_chunks);
  const long long rows = (long long)n - d, c0 = (long long)ch * MC_CHUNK;
  if (c0 >= rows && ch > 0) return;          // a chunk beyond the stratum: the fold does not read it
  long long c1 = c0 + MC_CHUNK;
  if (c1 > rows) c1 = rows;
  if (d < min_dist) c1 = c0;                 // a stratum below min_dist: no cell takes part
  const double* xa = Sa + (long long)d * ld;
  const double* xb = Sb + (long long)d * ld;
  double mx = 0.0, my = 0.0;
  if (pass_no == 2) mx = stats[2 * ((long long)D + 1) + d], my = stats[3 * ((long long)D + 1) + d];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  int cnt = 0;
  for (long long i = c0 + lane; i < c1; i += WAVE) {
    const double x = xa[i], y = xb[i];
    if (valid[i] && valid[i + d] && (x != 0.0 || y != 0.0)) {
      if (pass_no == 1) {
        s0 += x, s1 += y;
        ++cnt;
      } else {
        const double dx = x - mx, dy = y - my;
        s0 += dx * dx, s1 += dy * dy, s2 += dx * dy;
      }
    }
  }
  s0 = wave_sum_d(s0), s1 = wave_sum_d(s1), s2 = wave_sum_d(s2);
#pragma unroll
  for (int o = WAVE / 2; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o);
  if (lane == 0) {
    part[3 * w] = s0, part[3 * w + 1] = s1, part[3 * w + 2] = s2;
    part_n[w] = cnt;
  }
}

__global__ __launch_bounds__(MC_THREADS) void k_mapcmp_fold(int n, int D, int pass_no, int n_chunks,
                                                            const double* __restrict__ part, const int* __restrict__ part_n,
                                                            long long* __restrict__ cells, double* __restrict__ stats) {
  const long long d = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
  if (d > D) return;
  long long chunks = ((long long)n - d + MC_CHUNK - 1) / MC_CHUNK;   // chunk 0 is written for every stratum
  if (chunks < 1) chunks = 1;
  if (chunks > n_chunks) chunks = n_chunks;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  long long cnt = 0;
  for (long long c = 0; c < chunks; ++c) {
    const long long w = d * n_chunks + c;
    s0 += part[3 * w], s1 += part[3 * w + 1], s2 += part[3 * w + 2];
    cnt += part_n[w];
  }
  const long long L = (long long)D + 1;
  if (pass_no == 1) {
    cells[d] = cnt;
    stats[d] = s0, stats[L + d] = s1;
    stats[2 * L + d] = s0 / (double)cnt, stats[3 * L + d] = s1 / (double)cnt;   // NaN without cells: pass 2 adds nothing then
  } else {
    stats[4 * L + d] = s0, stats[5 * L + d] = s1, stats[6 * L + d] = s2;
  }
}

struct McPlan {
  int n_chunks;
  size_t part, part_n, total;
};

static McPlan mc_plan(int n, int D) {
  McPlan pl;
  pl.n_chunks = (int)tiles_of(n, MC_CHUNK);
  const long long waves = ((long long)D + 1) * pl.n_chunks;
  WsBump b = {0};
  pl.part = b.take((size_t)waves * 3 * sizeof(double));
  pl.part_n = b.take((size_t)waves * sizeof(int));
  pl.total = b.o + 256;
  return pl;
}

static size_t mc_lds_bytes(int h) {
  const size_t E = MC_T + 2 * (size_t)h;
  return (E * E + E * MC_T + 2 * E) * sizeof(double);
}

extern "C" {

int cgcn_mapcmp_smooth(cgcn_stream_t stream, int n, int D, int h, int width, const double* band, const double* norm,
                       long long n_norm, int ld, double* S) {
  if (n < 0 || D < 0 || h < 0 || width < 1 || n_norm < 0 || ld < n || (norm && n_norm < 1)) return CGCN_ERR_BAD_ARG;
  if (h > MC_HMAX || (long long)n * width > MC_MAX_ELEMS || ((long long)D + 1) * ld > MC_MAX_ELEMS) return CGCN_ERR_UNSUPPORTED;
  if ((long long)width < (long long)D + 2 * h + 1) return CGCN_ERR_BAD_ARG;
  if (ld > 0 && !S) return CGCN_ERR_BAD_ARG;
  if (n > 0 && !band) return CGCN_ERR_BAD_ARG;
  if (ld == 0) return CGCN_OK;
  const long long tiles_i = tiles_of(ld, MC_T), tiles_c = tiles_of((long long)MC_T + D, MC_T);
  hipLaunchKernelGGL(k_mapcmp_smooth, dim3((unsigned)(tiles_i * tiles_c)), dim3(MC_THREADS), mc_lds_bytes(h),
                     (hipStream_t)stream, n, D, h, width, band, norm, n_norm, ld, (int)tiles_c, S);
  return launch_status();
}

size_t cgcn_mapcmp_workspace_bytes(int n, int D) {
  if (n < 0 || D < 0 || ((long long)D + 1) * ((long long)n + 1) > MC_MAX_ELEMS) return 0;
  return mc_plan(n, D).total;
}

int cgcn_mapcmp_sums(cgcn_stream_t stream, int n, int D, int ld, const double* Sa, const double* Sb, const uint8_t* valid,
                     int min_dist, int pass_no, void* workspace, size_t workspace_bytes, long long* cells, double* stats) {
  if (n < 0 || D < 0 || ld < n || min_dist < 0 || (pass_no != 1 && pass_no != 2) || !workspace || !cells || !stats)
    return CGCN_ERR_BAD_ARG;
  if (((long long)D + 1) * ((long long)ld + 1) > MC_MAX_ELEMS) return CGCN_ERR_UNSUPPORTED;
  if (n > 0 && (!Sa || !Sb || !valid)) return CGCN_ERR_BAD_ARG;
  const McPlan pl = mc_plan(n, D);
  if (workspace_bytes < pl.total) return CGCN_ERR_WORKSPACE;
  char* base = ws_base(workspace);
  double* part = (double*)(base + pl.part);
  int* part_n = (int*)(base + pl.part_n);
  const long long waves = ((long long)D + 1) * pl.n_chunks;
  hipLaunchKernelGGL(k_mapcmp_sums, dim3((unsigned)tiles_of(waves, MC_THREADS / WAVE)), dim3(MC_THREADS), 0, (hipStream_t)stream,
                     n, D, ld, Sa, Sb, valid, min_dist, pass_no, pl.n_chunks, (const double*)stats, part, part_n);
  hipLaunchKernelGGL(k_mapcmp_fold, dim3((unsigned)tiles_of((long long)D + 1, MC_THREADS)), dim3(MC_THREADS), 0,
                     (hipStream_t)stream, n, D, pass_no, pl.n_chunks, (const double*)part, (const int*)part_n, cells, stats);
  return launch_status();
}

}  // extern "C"
