// chromegcn_amd/csrc/cgcn_hicmap.hpp
//
// What every analysis of a balanced Hi-C map reads the same way (chromegcn_amd/hicmap.py is the host side): a norm vector
// "as rule 1 reads it", the validity of a bin, and the start of a CSR row's upper part.  The fp64 wave and block sums that
// these kernels share with others live in cgcn_common.hpp.
#pragma once
#include "cgcn_common.hpp"

__device__ __forceinline__ double hm_inf() { return __longlong_as_double(0x7FF0000000000000ll); }
__device__ __forceinline__ double hm_nan() { return __longlong_as_double(0x7FF8000000000000ll); }   // the quiet NaN

// nv[b] of a norm vector of n_norm entries: NaN and 0 read as +inf, and so does a bin outside the vector (never out of
// bounds), so that a value divided by it is 0
__device__ __forceinline__ double hm_norm_at(const double* __restrict__ norm, long long n_norm, long long b) {
  if (b < 0 || b >= n_norm) return hm_inf();
  const double x = norm[b];
  return (x != x || x == 0.0) ? hm_inf() : x;
}

// the validity of bin b, 0 <= b < n (the caller's guarantee), and its norm value nv (1.0 without a vector): the bin has a
// positive row sum vc[b] and, with a vector, an entry there that is finite and not 0
__device__ __forceinline__ bool hm_bin(const double* __restrict__ vc, const double* __restrict__ norm, long long n_norm, long long b,
                                       double& nv) {
  nv = 1.0;
  bool ok = vc[b] > 0.0;
  if (norm) {
    if (b >= n_norm) return false;
    const double x = norm[b];
    ok = ok && x == x && x != 0.0 && __builtin_fabs(x) != hm_inf();
    nv = x;
  }
  return ok;
}

// the first entry of col[s..e) that is >= i (the columns of a CSR row ascend), e when there is none
__device__ __forceinline__ int hm_row_lower(const int* __restrict__ col, int s, int e, int i) {
  while (s < e) {
    const int mid = (int)(((long long)s + e) >> 1);
    if (col[mid] < i) s = mid + 1; else e = mid;
  }
  return s;
}
