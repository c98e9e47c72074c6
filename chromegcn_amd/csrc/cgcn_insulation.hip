// chromegcn_amd/csrc/cgcn_insulation.hip
//
// Diamond sums of one chromosome's contact matrix (chromegcn_amd/insulation.py holds the rule and its
// numpy restatement): S_w[i] = sum of A[a, b] / (nv[a] nv[b]) over a in [max(i - w, 0), i - 1], b in [i, min(i + w, n) - 1],
// the contacts across the junction left of bin i, for up to 8 window sizes w in one pass over the band.
//
//   k_insul_sums         a wavefront owns bin i (and i + the number of wavefronts, ...).  Lane l takes the rows a = i - 1 - l,
//                        i - 1 - l - 64, ... down to i - w_max: it finds the first column >= i of its row by binary search
//                        (the columns of a row are sorted) and walks the entries while the column is below i + w_max.  A term
//                        at (a, b) lies in the diamond of every window w >= max(i - a, b - i + 1) and is added to each of
//                        those accumulators.  One fixed butterfly over the lanes, then lane 0 stores the sums.
// A lane's terms come in (row, column) order and the butterfly is the same in every run: no floating-point atomic, no order
// that scheduling could change, so the same bits in every run and exact sums for integer counts below 2^53.  No workspace,
// nothing is allocated, nothing synchronises.
#include "cgcn_hicmap.hpp"

#define INS_THREADS 256
#define INS_MAX_WINDOWS 8
#define INS_MAX_BLOCKS 2048   // 8 workgroups per CU; the bins beyond are reached by the grid stride

struct InsWindows {
  int w[INS_MAX_WINDOWS];   // ascending; 0 behind the last one: no term is that close
};

__global__ __launch_bounds__(INS_THREADS) void k_insul_sums(int n, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                            const double* __restrict__ val, const double* __restrict__ norm,
                                                            long long n_norm, InsWindows win, int w_max, double* __restrict__ out) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long long waves = (long long)gridDim.x * (INS_THREADS / WAVE);
  for (long long bin = (long long)blockIdx.x * (INS_THREADS / WAVE) + threadIdx.x / WAVE; bin < n; bin += waves) {   // the whole wavefront
    const int i = (int)bin;
    const int lo = (int)max(bin - w_max, 0ll), hi = (int)min(bin + w_max, (long long)n);
    double acc[INS_MAX_WINDOWS];
#pragma unroll
    for (int k = 0; k < INS_MAX_WINDOWS; ++k) acc[k] = 0.0;
    for (int a = i - 1 - lane; a >= lo; a -= WAVE) {
      const int end = rowptr[a + 1];
      const int s = hm_row_lower(col, rowptr[a], end, i);   // the first entry of row a with a column >= i
      const double na = norm ? hm_norm_at(norm, n_norm, a) : 1.0;
      const int up = i - a;
      for (int p = s; p < end; ++p) {
        const int c = col[p];
        if (c >= hi) break;
        double v = val[p];
        if (norm) v = v / (na * hm_norm_at(norm, n_norm, c));   // one multiply, one divide; a NaN or 0 norm bin: the term is 0
        const int t = max(up, c - i + 1);
#pragma unroll
        for (int k = 0; k < INS_MAX_WINDOWS; ++k)
          if (t <= win.w[k]) acc[k] += v;
      }
    }
#pragma unroll
    for (int k = 0; k < INS_MAX_WINDOWS; ++k) acc[k] = wave_sum_d(acc[k]);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < INS_MAX_WINDOWS; ++k)
        if (win.w[k] > 0) out[(long long)k * n + bin] = acc[k];
    }
  }
}

extern "C" {

int cgcn_hicinsul_sums(cgcn_stream_t stream, int n, const int32_t* rowptr, const int32_t* col, const double* val,
                       const double* norm, long long n_norm, int n_windows, const int32_t* windows, double* out) {
  if (n < 0 || n_windows < 1 || n_norm < 0 || !rowptr || !windows) return CGCN_ERR_BAD_ARG;
  if (n > 0 && (!col || !val || !out)) return CGCN_ERR_BAD_ARG;
  if (norm && n_norm < 1) return CGCN_ERR_BAD_ARG;
  if (n_windows > INS_MAX_WINDOWS) return CGCN_ERR_UNSUPPORTED;
  InsWindows win;
  for (int k = 0; k < INS_MAX_WINDOWS; ++k) win.w[k] = 0;
  for (int k = 0; k < n_windows; ++k) {
    if (windows[k] < 1 || (k > 0 && windows[k] <= windows[k - 1])) return CGCN_ERR_BAD_ARG;
    win.w[k] = windows[k];
  }
  if (n == 0) return CGCN_OK;
  long long blocks = ((long long)n + INS_THREADS / WAVE - 1) / (INS_THREADS / WAVE);
  if (blocks > INS_MAX_BLOCKS) blocks = INS_MAX_BLOCKS;
  hipLaunchKernelGGL(k_insul_sums, dim3((unsigned)blocks), dim3(INS_THREADS), 0, (hipStream_t)stream, n, rowptr, col, val, norm,
                     n_norm, win, win.w[n_windows - 1], out);
  return launch_status();
}

}  // extern "C"
