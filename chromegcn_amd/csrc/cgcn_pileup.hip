// chromegcn_amd/csrc/cgcn_pileup.hip
//
// Pile-ups (aggregate peak analysis): the sum of a (2 w + 1)^2 window of the contact map around every centre of a list, per
// group (chromegcn_amd/pileup.py holds the rule and its numpy restatement).
//
//   k_pileup_values  the raw band of cgcn_hicloops_band -> the VALUE band: vband[a width + dd] is rule 1's value of the cell
//                    (a, a + dd), or a quiet NaN where the cell takes no part.  One thread per element, a grid-stride loop.
//                    Built once per map and value kind; the pile-up pass then costs one 8-byte read per cell and centre.
//   k_pileup_slices  a team of S^2 = (2 w + 1)^2 threads owns one slice of up to 256 consecutive centres of one group; thread t
//                    of the team owns the offset (da, db) = (t / S - w, t % S - w).  The team stages its centres in LDS (a
//                    centre that would reach outside the band is staged as "skip": the keep test is the caller's, the bounds
//                    are checked here again), then every thread walks the centres IN ORDER, four loads in flight, and keeps a
//                    double sum and an int count.  For a fixed da the S reads of a centre are contiguous.  A workgroup holds
//                    min(8, 512 / S^2) teams: 1 at w = 10, 4 at w = 5, 8 from w = 3 down.
//   k_pileup_fold    one thread per (g, da, db) adds that group's slice partials in slice order, eight loads in flight: with
//                    one group the S^2 threads are all there is, and the chain of dependent loads was the whole pile-up's
//                    longest step before they were batched.
// Every floating-point sum is sequential in a fixed order and there are no atomics: the same bits in every run.  Contraction
// is off, an fp64 division is IEEE here.
#include "cgcn_compact.hpp"
#include "cgcn_hicmap.hpp"

#pragma clang fp contract(off)

#define PU_WMAX 10
#define PU_SLICE 256
#define PU_THREADS 512
#define PU_MAX_TEAMS 8
#define PU_MAX_ELEMS (1ll << 28)
#define PU_MAX_GROUPS 65536
#define PU_VAL_THREADS 256

__global__ __launch_bounds__(PU_VAL_THREADS) void k_pileup_values(int n, int width, const double* __restrict__ band,
                                                                  const double* __restrict__ vc, const double* __restrict__ norm,
                                                                  long long n_norm, const double* __restrict__ ex, long long n_ex,
                                                                  int kind, double* __restrict__ vband) {
  const double nan = hm_nan(), inf = hm_inf();
  const long long total = (long long)n * width, step = (long long)gridDim.x * PU_VAL_THREADS;
  for (long long q = (long long)blockIdx.x * PU_VAL_THREADS + threadIdx.x; q < total; q += step) {
    const long long a = q / width, dd = q - a * width, b = a + dd;
    double out = nan;
    if (b < n) {
      double na, nb;
      bool part = hm_bin(vc, norm, n_norm, a, na);
      part = hm_bin(vc, norm, n_norm, b, nb) && part;
      if (part) {
        double v = band[q];
        if (kind >= CGCN_PILEUP_BALANCED) v = v / (na * nb);
        if (kind == CGCN_PILEUP_OE) {
          const double e = dd < n_ex ? ex[dd] : 0.0;
          part = e > 0.0;
          if (part) v = v / e;
        }
        if (part && v == v && __builtin_fabs(v) != inf) out = v;
      }
    }
    vband[q] = out;
  }
}

__global__ __launch_bounds__(PU_THREADS) void k_pileup_slices(int n, int width, const double* __restrict__ vband, int w, int teams,
                                                              int n_slices, const int* __restrict__ slice_off, long long m,
                                                              const int* __restrict__ ci, const int* __restrict__ cj,
                                                              double* __restrict__ part_sum, int* __restrict__ part_cnt) {
  __shared__ int2 cen[PU_MAX_TEAMS * PU_SLICE];
  __shared__ int len_s[PU_MAX_TEAMS];
  const int S = 2 * w + 1, SS = S * S, tid = threadIdx.x;
  const int team = tid / SS, t = tid - team * SS;
  const long long first = (long long)blockIdx.x * teams;
  // stage the centres of every team's slice; a centre whose window would leave the band is staged as (-1, -1)
  for (int k = 0; k < teams; ++k) {
    const long long s = first + k;
    int len = 0;
    if (s < n_slices) {
      long long lo = slice_off[s], hi = slice_off[s + 1];
      if (lo < 0) lo = 0;
      if (hi > m) hi = m;
      if (hi - lo > PU_SLICE) hi = lo + PU_SLICE;
      len = hi > lo ? (int)(hi - lo) : 0;
      for (int c = tid; c < len; c += blockDim.x) {
        int i = ci[lo + c], j = cj[lo + c];
        const long long d = (long long)j - i;
        if (i < w || (long long)j + w > (long long)n - 1 || d < 2 * w || d + 2 * w >= width) i = j = -1;
        cen[k * PU_SLICE + c] = make_int2(i, j);
      }
    }
    if (tid == 0) len_s[k] = len;
  }
  __syncthreads();
  const long long s = first + team;
  if (team >= teams || s >= n_slices) return;
  const int da = t / S - w, db = t - (t / S) * S - w;
  const int len = len_s[team];
  const int2* my = cen + team * PU_SLICE;
  const long long shift = (long long)da * width + (db - da);   // the cell's element minus the centre's
  double sum = 0.0;
  int cnt = 0;
  int c = 0;
  for (; c + 4 <= len; c += 4) {
    double v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int2 p = my[c + u];
      v[u] = p.x >= 0 ? vband[(long long)p.x * width + (p.y - p.x) + shift] : hm_nan();
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (v[u] == v[u]) sum += v[u], ++cnt;
  }
  for (; c < len; ++c) {
    const int2 p = my[c];
    if (p.x < 0) continue;
    const double v = vband[(long long)p.x * width + (p.y - p.x) + shift];
    if (v == v) sum += v, ++cnt;
  }
  part_sum[s * SS + t] = sum;
  part_cnt[s * SS + t] = cnt;
}

__global__ __launch_bounds__(PU_VAL_THREADS) void k_pileup_fold(int G, int SS, int n_slices, const int* __restrict__ group_off,
                                                                const double* __restrict__ part_sum,
                                                                const int* __restrict__ part_cnt, double* __restrict__ P,
                                                                long long* __restrict__ N) {
  const long long q = (long long)blockIdx.x * PU_VAL_THREADS + threadIdx.x;
  if (q >= (long long)G * SS) return;
  const int g = (int)(q / SS), t = (int)(q - (long long)g * SS);
  int lo = group_off[g], hi = group_off[g + 1];
  if (lo < 0) lo = 0;
  if (hi > n_slices) hi = n_slices;
  double sum = 0.0;
  long long cnt = 0;
  int s = lo;
  for (; s + 8 <= hi; s += 8) {   // eight partials in flight; the adds stay in slice order
    double v[8];
    int c[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      v[u] = part_sum[(long long)(s + u) * SS + t];
      c[u] = part_cnt[(long long)(s + u) * SS + t];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) sum += v[u], cnt += c[u];
  }
  for (; s < hi; ++s) {
    sum += part_sum[(long long)s * SS + t];
    cnt += part_cnt[(long long)s * SS + t];
  }
  P[q] = sum;
  N[q] = cnt;
}

struct PuPlan {
  size_t sum, cnt, total;
};

static PuPlan pu_plan(long long n_slices, int w) {
  const long long SS = (long long)(2 * w + 1) * (2 * w + 1);
  PuPlan pl;
  WsBump b = {0};
  pl.sum = b.take((size_t)(n_slices * SS) * sizeof(double));
  pl.cnt = b.take((size_t)(n_slices * SS) * sizeof(int));
  pl.total = b.o + 256;
  return pl;
}

extern "C" {

int cgcn_pileup_values(cgcn_stream_t stream, int n, int width, const double* band, const double* vc, const double* norm,
                       long long n_norm, const double* expected, long long n_expected, int kind, double* vband) {
  if (n < 0 || width < 1 || n_norm < 0 || n_expected < 0 || kind < CGCN_PILEUP_OBSERVED || kind > CGCN_PILEUP_OE)
    return CGCN_ERR_BAD_ARG;
  if ((long long)n * width > PU_MAX_ELEMS) return CGCN_ERR_UNSUPPORTED;
  if ((norm && n_norm < 1) || (kind == CGCN_PILEUP_OE && n_expected > 0 && !expected)) return CGCN_ERR_BAD_ARG;
  if (n > 0 && (!band || !vc || !vband)) return CGCN_ERR_BAD_ARG;
  if (n == 0) return CGCN_OK;
  long long blocks = tiles_of((long long)n * width, PU_VAL_THREADS);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(k_pileup_values, dim3((unsigned)blocks), dim3(PU_VAL_THREADS), 0, (hipStream_t)stream, n, width, band, vc,
                     norm, n_norm, expected, n_expected, kind, vband);
  return launch_status();
}

size_t cgcn_pileup_workspace_bytes(long long n_slices, int w) {
  if (n_slices < 0 || n_slices > (1ll << 24) || w < 1 || w > PU_WMAX) return 0;
  return pu_plan(n_slices, w).total;
}

int cgcn_pileup_slices(cgcn_stream_t stream, int n, int width, const double* vband, int w, long long n_slices,
                       const int32_t* slice_off, long long n_centres, const int32_t* ci, const int32_t* cj, void* workspace,
                       size_t workspace_bytes) {
  if (n < 0 || width < 1 || w < 1 || n_slices < 0 || n_centres < 0 || !workspace) return CGCN_ERR_BAD_ARG;
  if (w > PU_WMAX || n_slices > (1ll << 24) || (long long)n * width > PU_MAX_ELEMS) return CGCN_ERR_UNSUPPORTED;
  if (n_slices > 0 && (!vband || !slice_off)) return CGCN_ERR_BAD_ARG;
  if (n_centres > 0 && (!ci || !cj)) return CGCN_ERR_BAD_ARG;
  const PuPlan pl = pu_plan(n_slices, w);
  if (workspace_bytes < pl.total) return CGCN_ERR_WORKSPACE;
  if (n_slices == 0) return CGCN_OK;
  const int SS = (2 * w + 1) * (2 * w + 1);
  int teams = PU_THREADS / SS;
  if (teams > PU_MAX_TEAMS) teams = PU_MAX_TEAMS;
  const int threads = (teams * SS + WAVE - 1) / WAVE * WAVE;
  char* base = ws_base(workspace);
  hipLaunchKernelGGL(k_pileup_slices, dim3((unsigned)tiles_of(n_slices, teams)), dim3(threads), 0, (hipStream_t)stream, n, width,
                     vband, w, teams, (int)n_slices, slice_off, n_centres, ci, cj, (double*)(base + pl.sum),
                     (int*)(base + pl.cnt));
  return launch_status();
}

int cgcn_pileup_fold(cgcn_stream_t stream, int n_groups, int w, long long n_slices, const int32_t* group_off,
                     const void* workspace, size_t workspace_bytes, double* P, long long* N) {
  if (n_groups < 0 || w < 1 || n_slices < 0 || !workspace) return CGCN_ERR_BAD_ARG;
  if (w > PU_WMAX || n_groups > PU_MAX_GROUPS || n_slices > (1ll << 24)) return CGCN_ERR_UNSUPPORTED;
  if (n_groups > 0 && (!group_off || !P || !N)) return CGCN_ERR_BAD_ARG;
  const PuPlan pl = pu_plan(n_slices, w);
  if (workspace_bytes < pl.total) return CGCN_ERR_WORKSPACE;
  if (n_groups == 0) return CGCN_OK;
  const int SS = (2 * w + 1) * (2 * w + 1);
  const char* base = ws_base((void*)workspace);
  hipLaunchKernelGGL(k_pileup_fold, dim3((unsigned)tiles_of((long long)n_groups * SS, PU_VAL_THREADS)), dim3(PU_VAL_THREADS), 0,
                     (hipStream_t)stream, n_groups, SS, (int)n_slices, group_off, (const double*)(base + pl.sum),
                     (const int*)(base + pl.cnt), P, N);
  return launch_status();
}

}  // extern "C"
