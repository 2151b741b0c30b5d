// What the sensor-stage units under response tables share (rtx_srf.hip: rtx_srf_apply, rtx_srf_moments; rtx_srf_vjp.hip:
// their adjoint): the chunk and knot limits, the description of the axis and of a launch group's bands, and the device
// functions a row's weight w_b,i = R_b(X_i) D_i is formed with. One copy of each, so that the adjoint weighs a point with
// exactly the number the forward weighed it with.
#pragma once
#include "rtx_common.h"

#define SRF_CH 1024         // rows per chunk
#define SRF_MAX_KNOTS 1024  // per band: the knot table of one band is staged in LDS (12 KiB)
#define SRF_SLOTS 16        // bands per launch group = slots per chunk in the workspace

struct SrfArgs {
  GridDev g;
  const double* X;
  long long nx, nS, ldY;
  const float* Y;
  const double* kx;  // all bands' knots
  const float* kr;
  int ng;                  // bands in this group
  int ks[SRF_SLOTS + 1];   // their knot ranges [ks[j], ks[j + 1])
  long long* sup;   // [SRF_SLOTS][2] support [lo, hi) of each band as axis indices
  float* P;         // [n_chunks][SRF_SLOTS][nS] chunk sums
  double* W;        // [n_chunks][SRF_SLOTS] chunk sums of the weights
  float* Yout;      // the group's first row of Y_out
  float* wsum;      // NULL or the group's first denominator
};

__device__ __forceinline__ double srf_x(const SrfArgs& a, long long i) { return a.X ? a.X[i] : grid_x(a.g, a.g.offset + i); }

// trapezoid cell of point i on the axis passed
__device__ __forceinline__ double srf_delta(const SrfArgs& a, long long i) {
  if (a.nx == 1) return 1.0;
  const double xm = srf_x(a, i > 0 ? i - 1 : i), xp = srf_x(a, i < a.nx - 1 ? i + 1 : i);
  return 0.5 * (xp - xm);
}

// first index with X[i] > v (strict = 1) or X[i] >= v (strict = 0), X ascending (ils_bound's search)
__device__ long long srf_bound(const SrfArgs& a, double v, int strict) {
  long long lo = 0, hi = a.nx;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    const double x = srf_x(a, mid);
    const bool right = strict ? (x > v) : (x >= v);
    if (right) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// the segment of x among nk ascending knots: the largest j with kx[j] <= x, kept inside [0, nk - 2]
__device__ int srf_segment(const double* kx, int nk, double x) {
  int lo = 0, hi = nk;  // first index with kx > x
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (kx[mid] > x) hi = mid; else lo = mid + 1;
  }
  const int j = lo - 1;
  return j < 0 ? 0 : (j > nk - 2 ? nk - 2 : j);
}

// number of knots <= x
__device__ long long srfm_count(const double* Xk, long long nk, double x) {
  long long lo = 0, hi = nk;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (Xk[mid] > x) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// the weights (np.interp's hats) of a point x on the emissivity knots x0 <= x < x1 either side of it: each rounded to fp32
// once from the fp64 quotient. 1.0f - f from the rounded f is off by up to 2^-25 ABSOLUTELY, which next to the upper knot
// (f = 0.9963: a hat of 0.0037) is 130 x 2^-24 of the hat itself, and a band of a few such rows carries that into M.
__device__ __forceinline__ void srfm_hats(double x, double x0, double x1, float& h0, float& h1) {
  const double f = (x - x0) / (x1 - x0);
  h0 = (float)(1.0 - f);
  h1 = (float)f;
}

// the weight of row i under the band whose knots [0, m) are staged: srf_rows_kernel's, to the letter
__device__ __forceinline__ float srf_weight(const SrfArgs& a, const double* s_kx, const float* s_kr, int m, int& seg, long long i) {
  const double x = srf_x(a, i);
  while (seg + 2 < m && x >= s_kx[seg + 1]) ++seg;
  const double xa = s_kx[seg], xb = s_kx[seg + 1], ya = (double)s_kr[seg], yb = (double)s_kr[seg + 1];
  const double R = (yb - ya) / (xb - xa) * (x - xa) + ya;
  return (float)(fmax(R, 0.0) * srf_delta(a, i));
}
