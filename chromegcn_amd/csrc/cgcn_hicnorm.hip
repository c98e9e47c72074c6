// chromegcn_amd/csrc/cgcn_hicnorm.hip
//
// The KR / VC / SQRTVC normalisation vectors of a Hi-C contact matrix from the contact records themselves (DESIGN.md
// section 4.10; chromegcn_amd/hicnorm.py holds the definitions and their numpy restatement).
//
//   k_hn_keys            one pass over the M records: two 64-bit keys ((row << b | col) << rb | record, b = bits of n_bins,
//                        rb = bits of M) per record, the mirrored one a pad for a diagonal record; flags for a count that is
//                        negative or not finite, a negative position, a bin outside n_bins; the largest bin + 1
//   rocprim::radix_sort_keys    the record index is the low end of the key, so the records of one (row, col) come out in
//                        record order (keys alone: the (u64, u32) pair sort of rocprim 4 uses 80 B of scratch memory per
//                        lane on gfx950, which tests/test_kernel_resources.py does not let into the library);
//                        2 b + rb + 1 <= 64 is the price
//   k_hn_heads<false> / k_tile_scan / k_hn_heads<true>   an element starts an entry iff its key differs from the one before;
//                        the thread of a start walks its run and adds the counts IN RECORD ORDER: one ordered pass, the
//                        same bits in every run; columns, values, row pointers, the entry count
//   k_hn_spmv<STATS>     y = m o (A (m o x o p)) in fp64; a workgroup owns 16 consecutive rows: a row of at most
//                        `long_row_nnz` entries is summed by 16 lanes (four rows per wavefront) and a fixed shuffle tree, a
//                        longer one by the whole workgroup and a fixed tree in LDS.  No atomics.  STATS: the row sums (VC)
//                        and the number of positive entries per row instead
//   k_hn_vec / k_hn_finish   the vector work of one step of the Knight-Ruiz iteration with its scalars: per-workgroup
//                        partials, then one workgroup that folds them in a fixed order and updates the scalar record
// Nothing is allocated, nothing synchronises; loop control is the host's: every kernel does a bounded amount of work.
#include <cstring>  // rocprim 4.x headers use memset without including it
#include <rocprim/rocprim.hpp>

#include "cgcn_compact.hpp"
#include "cgcn_hicmap.hpp"

#define HN_THREADS 256
#define HN_ROWS 16                  // rows per workgroup of the product
#define HN_LONG_ROW 512             // default: rows with more entries take the workgroup route
#define HN_MAX_BLOCKS 1024          // workgroups of a vector step
#define HN_NPART 6                  // partial slots per workgroup: two sums, a minimum, a maximum, two more minima
#define HN_REC 32                   // doubles of the scalar record (CGCN_HICNORM_REC_*)
#define HN_HDR (HN_REC + HN_NPART * HN_MAX_BLOCKS)   // doubles in front of the vectors of the state
#define HN_VECTORS 11
#define HN_DELTA 0.1
#define HN_DELTA_UP 3.0

static inline size_t hn_stride(int n) { return ((size_t)(n < 1 ? 1 : n) + 31) & ~(size_t)31; }

// sizes[1] |= 1: a count that is negative or not finite; |= 2: a negative position; |= 4: a bin >= n_bins (n_bins > 0).
// A flagged record gets two pads: it is left out.  sizes[2] = the largest bin + 1 of the records with positions >= 0.
__global__ __launch_bounds__(HN_THREADS) void k_hn_keys(long long M, const int* __restrict__ pos1, const int* __restrict__ pos2,
                                                        const double* __restrict__ count, int res, long long n_bins, int b, int rb,
                                                        u64* __restrict__ keys, u64* sizes) {
  __shared__ unsigned wave_top[HN_THREADS / WAVE];
  const long long r = (long long)blockIdx.x * HN_THREADS + threadIdx.x;
  const u64 pad = (1ull << (2 * b)) << rb;
  unsigned bad = 0;
  long long top = 0;
  u64 k0 = pad, k1 = pad;
  if (r < M) {
    const int a = pos1[r], c = pos2[r];
    const double v = count[r];
    bad = (v >= 0.0 && v < hm_inf()) ? 0u : 1u;
    if (a < 0 || c < 0) {
      bad |= 2u;
    } else {
      const long long i = a / res, j = c / res;
      top = (i > j ? i : j) + 1;
      if (n_bins > 0 && top > n_bins) {
        bad |= 4u;
      } else if (!bad) {
        const u64 low = (u64)r & ((1ull << rb) - 1ull);   // rb = 0 (the count phase): the key is (row, col) alone
        k0 = ((((u64)i << b) | (u64)j) << rb) | low;
        if (i != j) k1 = ((((u64)j << b) | (u64)i) << rb) | low;
      }
    }
    keys[2 * r] = k0;
    keys[2 * r + 1] = k1;
  }
  // the maximum of the workgroup (shuffles, then LDS; every lane takes part; top <= 2^31), and an atomic only when it
  // exceeds the value already there: sorted dumps raise it a few times, not once per wavefront
  unsigned wtop = (unsigned)top;
#pragma unroll
  for (int o = WAVE / 2; o >= 1; o >>= 1) wtop = max(wtop, (unsigned)__shfl_xor((int)wtop, o));
  if ((threadIdx.x & (WAVE - 1)) == 0) wave_top[threadIdx.x / WAVE] = wtop;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned g = max(max(wave_top[0], wave_top[1]), max(wave_top[2], wave_top[3]));
    if ((u64)g > __atomic_load_n(&sizes[2], __ATOMIC_RELAXED)) atomicMax(&sizes[2], (u64)g);
  }
  if (bad) atomicOr(&sizes[1], (u64)bad);
}

// sorted keys [0, E), (row, col) = key >> rb: element e starts an entry iff it is no pad and its (row, col) differs from that
// of e - 1.  WRITE = false counts the starts per 256-element tile.  WRITE = true: the start at output place q < capacity writes its column and the sum of its run's counts
// in record order; it closes every row after the previous entry's up to its own (rowptr[r] = q); the last entry closes the
// rest with the entry count.
template <bool WRITE>
__global__ __launch_bounds__(HN_THREADS) void k_hn_heads(long long E, const u64* __restrict__ keys, const double* __restrict__ count,
                                                         int b, int rb, long long n_bins,
                                                         int* __restrict__ tile_counts, const long long* __restrict__ tile_off,
                                                         const int* __restrict__ total, long long capacity, int* __restrict__ rowptr,
                                                         int* __restrict__ col, double* __restrict__ val) {
  __shared__ int wave_tot[HN_THREADS / WAVE];
  const u64 pad = 1ull << (2 * b);
  const long long e = (long long)blockIdx.x * HN_THREADS + threadIdx.x;
  u64 k = pad, prev = pad;   // (row, col) of this element and of the one before
  bool head = false;
  if (e < E) {
    k = keys[e] >> rb;
    if (e > 0) prev = keys[e - 1] >> rb;
    head = k < pad && (e == 0 || k != prev);
  }
  const WgFlags<> heads(head, wave_tot);
  if (!WRITE) {
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = heads.count();
    return;
  }
  if (!head) return;
  const long long q = heads.before(tile_off[blockIdx.x]);
  const long long row = (long long)(k >> b);
  if (row >= n_bins) return;   // never: k_hn_keys pads such a record
  double s = 0.0;
  long long t = e;
  const u64 rmask = (1ull << rb) - 1ull;
  for (; t < E && (keys[t] >> rb) == k; ++t) s += count[keys[t] & rmask];
  if (q < capacity) {
    col[q] = (int)(k & ((1ull << b) - 1ull));
    val[q] = s;
  }
  // a capacity below the entry count truncates the matrix: no row pointer names a place col / val do not have
  const int qc = (int)(q < capacity ? q : capacity);
  const long long prow = e > 0 ? (long long)(prev >> b) : -1;   // e > 0: prev is an entry of an earlier or the same row
  for (long long r = prow + 1; r <= row; ++r) rowptr[r] = qc;
  if (t >= E || (keys[t] >> rb) >= pad) {
    const int tot = (int)(total[0] < capacity ? total[0] : capacity);
    for (long long r = row + 1; r <= n_bins; ++r) rowptr[r] = tot;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// y = m o (A (m o x o p)); m, x, p may each be NULL (= 1).  STATS: y = the row sums, nnz_out = positive entries per row.
__device__ __forceinline__ double hn_factor(const double* __restrict__ m, const double* __restrict__ x, const double* __restrict__ p,
                                            int j) {
  if (m && m[j] == 0.0) return 0.0;
  double f = 1.0;
  if (x) f = x[j];
  if (p) f *= p[j];
  return f;
}

template <bool STATS>
__global__ __launch_bounds__(HN_THREADS) void k_hn_spmv(int n, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                        const double* __restrict__ val, const double* __restrict__ m,
                                                        const double* __restrict__ x, const double* __restrict__ p,
                                                        double* __restrict__ y, int* __restrict__ nnz_out, int thr, int cap) {
  __shared__ double red[HN_THREADS];
  __shared__ int redc[HN_THREADS];
  const int row0 = blockIdx.x * HN_ROWS;
  // short rows: 16 lanes per row, four rows per wavefront
  {
    const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
    const int r = row0 + g;
    double acc = 0.0;
    int cnt = 0;
    bool mine = false;
    if (r < n) {
      const int b0 = min(rowptr[r], cap), e0 = min(rowptr[r + 1], cap);   // cap: the entries col / val hold
      mine = e0 - b0 <= thr;
      if (mine) {
        for (int q = b0 + l; q < e0; q += 16) {
          const double a = val[q];
          if (STATS) { acc += a; cnt += a > 0.0; }
          else acc += a * hn_factor(m, x, p, col[q]);
        }
      }
    }
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) {   // every lane of the wavefront takes part; the tree is the same for every row
      acc += __shfl_xor(acc, o, 16);
      if (STATS) cnt += __shfl_xor(cnt, o, 16);
    }
    if (mine && l == 0) {
      if (STATS) { y[r] = acc; nnz_out[r] = cnt; }
      else y[r] = (m && m[r] == 0.0) ? 0.0 : acc;
    }
  }
  // long rows: the whole workgroup, one row after the other
  for (int g = 0; g < HN_ROWS; ++g) {
    const int r = row0 + g;
    if (r >= n) break;
    const int b0 = min(rowptr[r], cap), e0 = min(rowptr[r + 1], cap);
    if (e0 - b0 <= thr) continue;   // the same for every thread of the workgroup
    double acc = 0.0;
    int cnt = 0;
    for (int q = b0 + (int)threadIdx.x; q < e0; q += HN_THREADS) {
      const double a = val[q];
      if (STATS) { acc += a; cnt += a > 0.0; }
      else acc += a * hn_factor(m, x, p, col[q]);
    }
    __syncthreads();
    red[threadIdx.x] = acc;
    if (STATS) redc[threadIdx.x] = cnt;
    __syncthreads();
    for (int s = HN_THREADS / 2; s >= 1; s >>= 1) {
      if ((int)threadIdx.x < s) {
        red[threadIdx.x] += red[threadIdx.x + s];
        if (STATS) redc[threadIdx.x] += redc[threadIdx.x + s];
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      if (STATS) { y[r] = red[0]; nnz_out[r] = redc[0]; }
      else y[r] = (m && m[r] == 0.0) ? 0.0 : red[0];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The state of one Knight-Ruiz run: [HN_REC scalars][HN_NPART x HN_MAX_BLOCKS partials][11 vectors of hn_stride(n)]
enum { HN_M = 0, HN_X, HN_V, HN_P, HN_W, HN_Y0, HN_Y1, HN_RK0, HN_RK1, HN_Z0, HN_Z1 };
enum { OP_MASK = 0, OP_RES, OP_FIRST, OP_DIR, OP_W, OP_Y, OP_CLIP, OP_COUNT };
// the record: 0 rho1, 1 rho2, 2 p.w, 3 min ynew, 4 max ynew, 5 gamma (lower bound), 6 gamma (upper bound), 7 rho1 of the
// accepted step, 8 rout, 9 alpha, 10 kept rows, 11 non-empty rows

__global__ __launch_bounds__(HN_THREADS) void k_hn_vec(int n, int op, int flag, int c, const double* __restrict__ vc,
                                                       const int* __restrict__ row_nnz, double* __restrict__ st, size_t ns) {
  __shared__ double red[HN_NPART][HN_THREADS];
  const double* rec = st;
  double* vec = st + HN_HDR;
  double* m = vec + HN_M * ns;
  double* x = vec + HN_X * ns;
  double* v = vec + HN_V * ns;
  double* p = vec + HN_P * ns;
  double* w = vec + HN_W * ns;
  double* y = vec + (HN_Y0 + c) * ns;
  double* y2 = vec + (HN_Y0 + (c ^ 1)) * ns;
  double* rk = vec + (HN_RK0 + c) * ns;
  double* rk2 = vec + (HN_RK0 + (c ^ 1)) * ns;
  double* Z = vec + (HN_Z0 + c) * ns;
  double* Z2 = vec + (HN_Z0 + (c ^ 1)) * ns;
  double s0 = 0.0, s1 = 0.0, mn0 = hm_inf(), mx0 = -hm_inf(), mn1 = hm_inf(), mn2 = hm_inf();
  const double beta = op == OP_DIR ? rec[7] / rec[0] : 0.0;
  const double alpha = rec[9];
  const double gamma = op == OP_CLIP ? rec[flag ? 6 : 5] : 0.0;
  const int step = gridDim.x * HN_THREADS;
  for (int i = blockIdx.x * HN_THREADS + threadIdx.x; i < n; i += step) {
    switch (op) {
      case OP_MASK: {
        const bool full = vc[i] > 0.0;
        const bool keep = full && row_nnz[i] >= flag;
        m[i] = keep ? 1.0 : 0.0;
        x[i] = 1.0;
        y[i] = 1.0;
        s0 += keep ? 1.0 : 0.0;
        s1 += full ? 1.0 : 0.0;
        break;
      }
      case OP_RES: {
        double xi = x[i];
        if (flag) { xi *= y[i]; x[i] = xi; }
        const double vi = xi * w[i];
        const double r = m[i] != 0.0 ? 1.0 - vi : 0.0;
        v[i] = vi;
        rk[i] = r;
        y[i] = 1.0;
        s0 += r * r;
        break;
      }
      case OP_FIRST: {
        const double r = rk[i];
        const double z = m[i] != 0.0 ? r / v[i] : 0.0;
        Z[i] = z;
        p[i] = z;
        s0 += r * z;
        break;
      }
      case OP_DIR:
        p[i] = Z[i] + beta * p[i];
        break;
      case OP_W: {
        const double pi = p[i];
        const double wi = x[i] * w[i] + v[i] * pi;
        w[i] = wi;
        s0 += pi * wi;
        break;
      }
      case OP_Y: {
        const double ap = alpha * p[i], yi = y[i];
        const double yn = yi + ap;
        y2[i] = yn;
        const double r = rk[i] - alpha * w[i];
        const bool keep = m[i] != 0.0;
        const double z = keep ? r / v[i] : 0.0;
        rk2[i] = r;
        Z2[i] = z;
        s0 += r * z;
        if (keep) {
          mn0 = fmin(mn0, yn);
          mx0 = fmax(mx0, yn);
          if (ap < 0.0) mn1 = fmin(mn1, (HN_DELTA - yi) / ap);
          if (yn > HN_DELTA_UP) mn2 = fmin(mn2, (HN_DELTA_UP - yi) / ap);
        }
        break;
      }
      default:   // OP_CLIP
        y[i] += gamma * (alpha * p[i]);
        break;
    }
  }
  if (op == OP_DIR || op == OP_CLIP) return;
  const int t = threadIdx.x;
  red[0][t] = s0; red[1][t] = s1; red[2][t] = mn0; red[3][t] = mx0; red[4][t] = mn1; red[5][t] = mn2;
  __syncthreads();
  for (int s = HN_THREADS / 2; s >= 1; s >>= 1) {
    if (t < s) {
      red[0][t] += red[0][t + s];
      red[1][t] += red[1][t + s];
      red[2][t] = fmin(red[2][t], red[2][t + s]);
      red[3][t] = fmax(red[3][t], red[3][t + s]);
      red[4][t] = fmin(red[4][t], red[4][t + s]);
      red[5][t] = fmin(red[5][t], red[5][t + s]);
    }
    __syncthreads();
  }
  if (t < HN_NPART) st[HN_REC + (size_t)blockIdx.x * HN_NPART + t] = red[t][0];
}

// one workgroup: the partials of `nblk` workgroups in a fixed order, then the step's update of the record
__global__ __launch_bounds__(HN_THREADS) void k_hn_finish(int nblk, int op, int flag, double* __restrict__ st) {
  __shared__ double red[HN_NPART][HN_THREADS];
  const double* part = st + HN_REC;
  const int t = threadIdx.x;
  double s0 = 0.0, s1 = 0.0, mn0 = hm_inf(), mx0 = -hm_inf(), mn1 = hm_inf(), mn2 = hm_inf();
  for (int b = t; b < nblk; b += HN_THREADS) {
    const double* q = part + (size_t)b * HN_NPART;
    s0 += q[0];
    s1 += q[1];
    mn0 = fmin(mn0, q[2]);
    mx0 = fmax(mx0, q[3]);
    mn1 = fmin(mn1, q[4]);
    mn2 = fmin(mn2, q[5]);
  }
  red[0][t] = s0; red[1][t] = s1; red[2][t] = mn0; red[3][t] = mx0; red[4][t] = mn1; red[5][t] = mn2;
  __syncthreads();
  for (int s = HN_THREADS / 2; s >= 1; s >>= 1) {
    if (t < s) {
      red[0][t] += red[0][t + s];
      red[1][t] += red[1][t + s];
      red[2][t] = fmin(red[2][t], red[2][t + s]);
      red[3][t] = fmax(red[3][t], red[3][t + s]);
      red[4][t] = fmin(red[4][t], red[4][t + s]);
      red[5][t] = fmin(red[5][t], red[5][t + s]);
    }
    __syncthreads();
  }
  if (t != 0) return;
  double* rec = st;
  switch (op) {
    case OP_MASK: rec[10] = red[0][0]; rec[11] = red[1][0]; break;
    case OP_RES: rec[0] = red[0][0]; rec[8] = red[0][0]; break;
    case OP_FIRST: rec[0] = red[0][0]; break;
    case OP_W:
      if (flag) { rec[1] = rec[0]; rec[0] = rec[7]; }   // the step before was accepted: rho2 = rho1, rho1 = its rk . Z
      rec[2] = red[0][0];
      rec[9] = rec[0] / red[0][0];
      break;
    case OP_Y:
      rec[3] = red[2][0]; rec[4] = red[3][0]; rec[5] = red[4][0]; rec[6] = red[5][0]; rec[7] = red[0][0];
      break;
    default: break;
  }
}

// kind 0: VC, 1: SQRTVC, 2: KR (1 / x on the kept rows); NaN on every other row
__global__ __launch_bounds__(HN_THREADS) void k_hn_vector(int n, int kind, const double* __restrict__ vc, const double* __restrict__ st,
                                                          size_t ns, double* __restrict__ out) {
  const int i = blockIdx.x * HN_THREADS + threadIdx.x;
  if (i >= n) return;
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  double r = nan;
  if (kind == 2) {
    const double* vec = st + HN_HDR;
    if (vec[HN_M * ns + i] != 0.0) r = 1.0 / vec[HN_X * ns + i];
  } else if (vc[i] > 0.0) {
    r = kind == 1 ? sqrt(vc[i]) : vc[i];
  }
  out[i] = r;
}

struct HnPlan {
  long long E, tiles;
  int b, rb;   // n_bins = 0 (the count phase): rb = 0, the keys carry no record index
  size_t temp, o_sizes, o_counts, o_off, o_keyA, o_keyB, o_temp, total;
};

static bool hn_plan(long long M, long long n_bins, HnPlan* p) {
  if (M < 0 || n_bins < 0 || M >= 2147483647ll || n_bins >= 2147483647ll) return false;
  p->E = 2 * (M < 1 ? 1 : M);
  p->tiles = tiles_of(p->E, HN_THREADS);
  p->b = n_bins > 0 ? bits_for(n_bins) : 31;
  p->rb = n_bins > 0 ? bits_for(M) : 0;
  if (2 * p->b + p->rb + 1 > 64) return false;
  size_t t = 0;
  (void)rocprim::radix_sort_keys(nullptr, t, (const u64*)nullptr, (u64*)nullptr, (size_t)p->E, 0u, (unsigned)(2 * p->b + p->rb + 1));
  p->temp = t;
  WsBump w = {0};
  p->o_sizes = w.take(256);
  p->o_counts = w.take((size_t)p->tiles * 4);
  p->o_off = w.take((size_t)p->tiles * 8);
  p->o_keyA = w.take((size_t)p->E * 8);
  p->o_keyB = w.take((size_t)p->E * 8);
  p->o_temp = w.take(p->temp);
  p->total = w.o + 256;   // the base is rounded up to 256 bytes
  return true;
}

// keys, sort, entry count: what both phases share.  sizes[0..3) are written.
static int hn_sorted(hipStream_t st, const HnPlan& p, char* w, long long M, const int32_t* pos1, const int32_t* pos2,
                     const double* count, int res, long long n_bins, u64* sizes, int* total32) {
  u64* keyA = (u64*)(w + p.o_keyA);
  u64* keyB = (u64*)(w + p.o_keyB);
  int* counts = (int*)(w + p.o_counts);
  long long* off = (long long*)(w + p.o_off);
  const long long E = 2 * M;
  if (hipMemsetAsync(sizes, 0, 32, st) != hipSuccess) return CGCN_ERR_LAUNCH;
  hipLaunchKernelGGL(k_hn_keys, dim3((unsigned)tiles_of(M, HN_THREADS)), dim3(HN_THREADS), 0, st, M, pos1, pos2, count, res, n_bins, p.b,
                     p.rb, keyA, sizes);
  size_t temp = p.temp;
  if (rocprim::radix_sort_keys((void*)(w + p.o_temp), temp, (const u64*)keyA, keyB, (size_t)E, 0u, (unsigned)(2 * p.b + p.rb + 1), st) !=
      hipSuccess)
    return CGCN_ERR_LAUNCH;
  hipLaunchKernelGGL(k_hn_heads<false>, dim3((unsigned)tiles_of(E, HN_THREADS)), dim3(HN_THREADS), 0, st, E, (const u64*)keyB, count, p.b,
                     p.rb, n_bins, counts, (const long long*)nullptr, (const int*)nullptr, 0ll, (int*)nullptr, (int*)nullptr,
                     (double*)nullptr);
  hipLaunchKernelGGL(k_tile_scan<>, dim3(1), dim3(1024), 0, st, (int)tiles_of(E, HN_THREADS), (const int*)counts, off,
                     (long long*)sizes, total32, 2147483647ll);
  return CGCN_OK;
}

static int hn_blocks(int n) {
  const long long k = tiles_of(n, HN_THREADS);
  return (int)(k < HN_MAX_BLOCKS ? k : HN_MAX_BLOCKS);
}

extern "C" {

size_t cgcn_hicnorm_workspace_bytes(long long M, long long n_bins) {
  HnPlan p;
  return hn_plan(M, n_bins, &p) ? p.total : 0;
}

int cgcn_hicnorm_count(cgcn_stream_t stream, long long M, const int32_t* pos1, const int32_t* pos2, const double* count,
                       int resolution_bp, long long n_bins, void* workspace, size_t workspace_bytes, long long* sizes) {
  if (M < 0 || n_bins < 0 || resolution_bp < 1 || !sizes || !workspace) return CGCN_ERR_BAD_ARG;
  if (M > 0 && (!pos1 || !pos2 || !count)) return CGCN_ERR_BAD_ARG;
  HnPlan p;
  if (!hn_plan(M, n_bins, &p)) return CGCN_ERR_UNSUPPORTED;
  if (workspace_bytes < p.total) return CGCN_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (M == 0) return hipMemsetAsync(sizes, 0, 32, st) == hipSuccess ? CGCN_OK : CGCN_ERR_LAUNCH;
  char* w = ws_base(workspace);
  const int rc = hn_sorted(st, p, w, M, pos1, pos2, count, resolution_bp, n_bins, (u64*)sizes, (int*)nullptr);
  return rc != CGCN_OK ? rc : launch_status();
}

int cgcn_hicnorm_fill(cgcn_stream_t stream, long long M, const int32_t* pos1, const int32_t* pos2, const double* count,
                      int resolution_bp, long long n_bins, long long capacity, void* workspace, size_t workspace_bytes,
                      int32_t* rowptr, int32_t* col, double* val, double* vc, int32_t* row_nnz, long long* sizes) {
  if (M < 0 || n_bins < 1 || capacity < 0 || resolution_bp < 1 || !sizes || !workspace || !rowptr || !vc || !row_nnz)
    return CGCN_ERR_BAD_ARG;
  if (M > 0 && (!pos1 || !pos2 || !count)) return CGCN_ERR_BAD_ARG;
  if (capacity > 0 && (!col || !val)) return CGCN_ERR_BAD_ARG;
  HnPlan p;
  if (!hn_plan(M, n_bins, &p) || capacity >= 2147483647ll) return CGCN_ERR_UNSUPPORTED;
  if (workspace_bytes < p.total) return CGCN_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* w = ws_base(workspace);
  const int n = (int)n_bins;
  if (hipMemsetAsync(rowptr, 0, ((size_t)n + 1) * 4, st) != hipSuccess) return CGCN_ERR_LAUNCH;
  if (M == 0) {
    if (hipMemsetAsync(sizes, 0, 32, st) != hipSuccess) return CGCN_ERR_LAUNCH;
  } else {
    int* total32 = (int*)(w + p.o_sizes);
    const int rc = hn_sorted(st, p, w, M, pos1, pos2, count, resolution_bp, n_bins, (u64*)sizes, total32);
    if (rc != CGCN_OK) return rc;
    const long long E = 2 * M;
    hipLaunchKernelGGL(k_hn_heads<true>, dim3((unsigned)tiles_of(E, HN_THREADS)), dim3(HN_THREADS), 0, st, E,
                       (const u64*)(w + p.o_keyB), count, p.b, p.rb, n_bins, (int*)nullptr, (const long long*)(w + p.o_off),
                       (const int*)total32, capacity, rowptr, col, val);
  }
  hipLaunchKernelGGL(k_hn_spmv<true>, dim3((unsigned)((n + HN_ROWS - 1) / HN_ROWS)), dim3(HN_THREADS), 0, st, n, (const int*)rowptr,
                     (const int*)col, (const double*)val, (const double*)nullptr, (const double*)nullptr, (const double*)nullptr, vc,
                     row_nnz, HN_LONG_ROW, (int)capacity);
  return launch_status();
}

int cgcn_hicnorm_spmv(cgcn_stream_t stream, int n, const int32_t* rowptr, const int32_t* col, const double* val,
                      const double* mask, const double* x, const double* p, double* y, int long_row_nnz) {
  if (n < 0) return CGCN_ERR_BAD_ARG;
  if (n == 0) return CGCN_OK;
  if (!rowptr || !col || !val || !y) return CGCN_ERR_BAD_ARG;
  const int thr = long_row_nnz < 0 ? HN_LONG_ROW : long_row_nnz;
  hipLaunchKernelGGL(k_hn_spmv<false>, dim3((unsigned)((n + HN_ROWS - 1) / HN_ROWS)), dim3(HN_THREADS), 0, (hipStream_t)stream, n, rowptr,
                     col, val, mask, x, p, y, (int*)nullptr, thr, 2147483647);
  return launch_status();
}

size_t cgcn_hicnorm_kr_state_bytes(int n) {
  if (n < 1) return 0;
  return ((size_t)HN_HDR + (size_t)HN_VECTORS * hn_stride(n)) * sizeof(double);
}

int cgcn_hicnorm_kr_step(cgcn_stream_t stream, int n, int op, int flag, int parity, const double* vc, const int32_t* row_nnz,
                         void* state, size_t state_bytes) {
  if (n < 1 || op < 0 || op >= OP_COUNT || (parity != 0 && parity != 1) || !state || ((uintptr_t)state & 7)) return CGCN_ERR_BAD_ARG;
  if (op == OP_MASK && (!vc || !row_nnz)) return CGCN_ERR_BAD_ARG;
  if (state_bytes < cgcn_hicnorm_kr_state_bytes(n)) return CGCN_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = hn_blocks(n);
  hipLaunchKernelGGL(k_hn_vec, dim3((unsigned)nblk), dim3(HN_THREADS), 0, st, n, op, flag, parity, vc, (const int*)row_nnz, (double*)state,
                     hn_stride(n));
  if (op != OP_DIR && op != OP_CLIP)
    hipLaunchKernelGGL(k_hn_finish, dim3(1), dim3(HN_THREADS), 0, st, nblk, op, flag, (double*)state);
  return launch_status();
}

int cgcn_hicnorm_vector(cgcn_stream_t stream, int n, int kind, const double* vc, const void* state, double* out) {
  if (n < 0 || kind < 0 || kind > 2) return CGCN_ERR_BAD_ARG;
  if (n == 0) return CGCN_OK;
  if (!out || (kind == 2 ? !state : !vc)) return CGCN_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_hn_vector, dim3((unsigned)tiles_of(n, HN_THREADS)), dim3(HN_THREADS), 0, (hipStream_t)stream, n, kind, vc,
                     (const double*)state, hn_stride(n), out);
  return launch_status();
}

}  // extern "C"
