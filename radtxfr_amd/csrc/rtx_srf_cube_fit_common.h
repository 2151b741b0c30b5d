// What the per-pixel fit kernels share (rtx_srf_cube_fit.hip, rtx_srf_cube_fit_box.hip): the argument
// block, a pixel's sums, one evaluation (scf_eval), the damped Cholesky step (scf_solve), the trial point (scf_trial) and
// the checks both families of entries make before their own (scf_front). SCF_PB (pixels per workgroup: one wave) and
// SCF_TAB_LDS (nEnd * Q up to which the table slice lives in LDS) are defined in rtx_srf_cube_fit.hip before it includes this
// file; any other file takes them from here, and the assertion below keeps the two from drifting apart.
#pragma once
#include "rtx_common.h"
#include "rtx_srf_cube_common.h"

#ifndef SCF_PB
#define SCF_PB 64
#endif
#ifndef SCF_TAB_LDS
#define SCF_TAB_LDS 128
#endif
static_assert(SCF_PB == 64 && SCF_TAB_LDS == 128, "lane = pixel in ONE wave of 64, and the sibling kernels' LDS threshold: every includer must agree");

#define SCF_QMAX 8       // rtx_srf_cube_max_nodes()
#define SCF_MIX_MAX 4    // rtx_srf_pixel_cube_fit_max_mix(): every instantiation without scratch (profiles/cube_fit_resources.txt)
#define SCF_ITER_MAX 1000
#define SCF_LAM_MIN 1e-12
#define SCF_LAM_MAX 1e12

struct ScfArgs {
  int nB, nEnd;
  long long nPix;
  double Tn[SCF_QMAX];   // the nodes
  double den[SCF_QMAX];  // prod_{r != q} (T_q - T_r), r ascending
  double T_lo, T_hi;
  const float *N, *C;
  const float* tab;    // [nEnd][Q][nB]
  const int* kidx;     // [nPix][nMix]
  const float* meas;   // [nB][nPix]
  const float* wgt;    // [nB] or NULL
  int stride;          // words per band of the LDS slice; 0: the table is read from global memory
  // normal
  const float* frac_in;
  const double* T_in;
  const double* lambda;  // [nPix] or NULL
  double *grad, *step;
  // fit
  float* frac;
  double* Tpix;
  int max_iter, given;
  double lambda0, ftol;
  int *n_iter, *status;
  // both
  double *cost, *hess;
};

template <int NM>
struct ScfSums {
  static constexpr int NU = NM + 1, NH = (NM + 1) * (NM + 2) / 2;
  double c, g[NU], H[NH];
};

__host__ __device__ constexpr int scf_tri(int i, int j) { return i * (i + 1) / 2 + j; }  // i >= j

// One evaluation at (T, f) for the lane's pixel p (clamped into the scene by the caller). Called by every thread of the
// workgroup together: the LDS slice is restaged per block of 64 bands.
template <int Q, int NM>
__device__ __forceinline__ void scf_eval(const ScfArgs& a, float* s_tab, long long p, double T, const float (&f)[NM], const int (&k)[NM],
                                         ScfSums<NM>& o) {
  constexpr int NU = NM + 1;
  float w[Q], wp[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    double l, dl;
    srf_cube_weight<Q>(a, T, q, l, dl);
    w[q] = (float)l;
    wp[q] = (float)dl;
  }
  o.c = 0.0;
#pragma unroll
  for (int i = 0; i < NU; ++i) o.g[i] = 0.0;
#pragma unroll
  for (int i = 0; i < ScfSums<NM>::NH; ++i) o.H[i] = 0.0;
  const int S = a.stride, rows = a.nEnd * Q;
  for (int b0 = 0; b0 < a.nB; b0 += 64) {
    const int nb = min(64, a.nB - b0);
    if (S) {
      __syncthreads();  // the last block's slice is read
      for (int i = threadIdx.x; i < rows * 64; i += SCF_PB) {
        const int kq = i >> 6, bl = i & 63;
        if (bl < nb) s_tab[bl * S + kq] = a.tab[(size_t)kq * a.nB + b0 + bl];
      }
      __syncthreads();
    }
    for (int bl = 0; bl < nb; ++bl) {
      const int b = b0 + bl;
      const float Nb = a.N[b];
      const float wb = a.wgt ? a.wgt[b] : 1.f;
      if (!(Nb > 0.f && wb > 0.f)) continue;  // uniform: a band that does not count is never read
      const float Cb = a.C[b];
      const float ms = a.meas[(size_t)b * (size_t)a.nPix + (size_t)p];
      const double invN = 1.0 / (double)Nb;
      double j[NU];
      float s = 0.f;
      double sT = 0.0;
#pragma unroll
      for (int m = 0; m < NM; ++m) {
        float G[Q];
        if (S) {
          const float* row = s_tab + bl * S + k[m] * Q;
          if (Q % 4 == 0) {
#pragma unroll
            for (int v = 0; v < Q / 4; ++v) {
              const float4 x = reinterpret_cast<const float4*>(row)[v];
              G[4 * v] = x.x; G[4 * v + 1] = x.y; G[4 * v + 2] = x.z; G[4 * v + 3] = x.w;
            }
          } else {
#pragma unroll
            for (int q = 0; q < Q; ++q) G[q] = row[q];
          }
        } else {
          const float* row = a.tab + (size_t)k[m] * Q * a.nB + b;
#pragma unroll
          for (int q = 0; q < Q; ++q) G[q] = row[(size_t)q * a.nB];
        }
        float t = 0.f, tp = 0.f;
#pragma unroll
        for (int q = 0; q < Q; ++q) { t = fmaf(w[q], G[q], t); tp = fmaf(wp[q], G[q], tp); }
        s = fmaf(f[m], t, s);
        sT = fma((double)f[m], (double)tp, sT);
        j[m + 1] = invN * (double)t;
      }
      j[0] = invN * sT;
      const float y = (Cb + s) / Nb;
      const double r = (double)y - (double)ms;
      const double wd = (double)wb, wr = wd * r;
      o.c = fma(wr, r, o.c);
#pragma unroll
      for (int i = 0; i < NU; ++i) {
        o.g[i] = fma(j[i], wr, o.g[i]);
        const double wj = wd * j[i];
#pragma unroll
        for (int jj = 0; jj <= i; ++jj) o.H[scf_tri(i, jj)] = fma(wj, j[jj], o.H[scf_tri(i, jj)]);
      }
    }
  }
}

// (H + lam diag H) d = -g over the unknowns OFF .. OFF + N - 1 of an NM-mixture's sums. False: a pivot was not finite or
// not positive, d is NaN.
template <int NM, int OFF, int N>
__device__ __forceinline__ bool scf_solve(const ScfSums<NM>& s, double lam, double (&d)[N]) {
  double L[N * (N + 1) / 2];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const double hjj = s.H[scf_tri(j + OFF, j + OFF)];
    double piv = fma(lam, hjj, hjj);
#pragma unroll
    for (int kk = 0; kk < j; ++kk) piv = fma(-L[scf_tri(j, kk)], L[scf_tri(j, kk)], piv);
    ok = ok && piv > 0.0 && piv <= 1.79769313486231570815e308;  // false for NaN and infinity
    const double ljj = sqrt(piv);
    L[scf_tri(j, j)] = ljj;
#pragma unroll
    for (int i = j + 1; i < N; ++i) {
      double v = s.H[scf_tri(i + OFF, j + OFF)];
#pragma unroll
      for (int kk = 0; kk < j; ++kk) v = fma(-L[scf_tri(i, kk)], L[scf_tri(j, kk)], v);
      L[scf_tri(i, j)] = v / ljj;
    }
  }
  double z[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double v = -s.g[i + OFF];
#pragma unroll
    for (int kk = 0; kk < i; ++kk) v = fma(-L[scf_tri(i, kk)], z[kk], v);
    z[i] = v / L[scf_tri(i, i)];
  }
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    double v = z[i];
#pragma unroll
    for (int kk = N - 1; kk > i; --kk) v = fma(-L[scf_tri(kk, i)], d[kk], v);
    d[i] = v / L[scf_tri(i, i)];
  }
  if (!ok) {
#pragma unroll
    for (int i = 0; i < N; ++i) d[i] = __builtin_nan("");
  }
  return ok;
}

// The trial point of a step d from (T, f): T clamped into the range, the fractions rounded to fp32 once.
template <int NM>
__device__ __forceinline__ void scf_trial(const ScfArgs& a, double T, const float (&f)[NM], const double (&d)[NM + 1], double& Tt,
                                          float (&ft)[NM]) {
  double x = T + d[0];
  x = x < a.T_lo ? a.T_lo : x;
  Tt = x > a.T_hi ? a.T_hi : x;
#pragma unroll
  for (int m = 0; m < NM; ++m) ft[m] = (float)((double)f[m] + d[m + 1]);
}

// What the entries check and fill in before their own arguments. 0: go on; 1: refused (RTX_FAIL has the message).
static int scf_front(const char* fn, ScfArgs& a, int nB, int Q, const double* T_node_h, int nEnd, int64_t nPix, int nMix) {
  memset(&a, 0, sizeof(a));
  if (Q < 1 || Q > SCF_QMAX) RTX_FAIL("%s: Q=%d outside [1,%d]", fn, Q, SCF_QMAX);
  if (nB < 0 || nPix < 0) RTX_FAIL("%s: negative size", fn);
  if (nEnd < 1 || nMix < 1) RTX_FAIL("%s: nEnd=%d, nMix=%d: need at least 1 of each", fn, nEnd, nMix);
  if (nMix > SCF_MIX_MAX) RTX_FAIL("%s: nMix=%d above rtx_srf_pixel_cube_fit_max_mix() = %d", fn, nMix, SCF_MIX_MAX);
  if (!T_node_h) RTX_FAIL("%s: a required pointer is NULL", fn);
  a.T_lo = T_node_h[Q]; a.T_hi = T_node_h[Q + 1];
  if (!(a.T_lo > 0.0) || !isfinite(a.T_hi) || !(a.T_lo <= a.T_hi)) RTX_FAIL("%s: temperature range [%g, %g]", fn, a.T_lo, a.T_hi);
  for (int q = 0; q < SCF_QMAX; ++q) { a.Tn[q] = 0.0; a.den[q] = 1.0; }
  for (int q = 0; q < Q; ++q) {
    const double T = T_node_h[q];
    if (!isfinite(T) || !(T > 0.0)) RTX_FAIL("%s: node temperature %g", fn, T);
    if (T < a.T_lo || T > a.T_hi) RTX_FAIL("%s: node temperature %g outside the range [%g, %g]", fn, T, a.T_lo, a.T_hi);
    a.Tn[q] = T;
  }
  for (int q = 0; q < Q; ++q) {
    double den = 1.0;
    for (int r = 0; r < Q; ++r)
      if (r != q) den *= a.Tn[q] - a.Tn[r];
    if (den == 0.0 || !isfinite(den)) RTX_FAIL("%s: the node temperatures are not distinct (node %d: %g)", fn, q, a.Tn[q]);
    a.den[q] = den;
  }
  if ((nPix + SCF_PB - 1) / SCF_PB > 0x7fffffffLL) RTX_FAIL("%s: nPix=%lld: too many pixels for one call", fn, (long long)nPix);
  a.nB = nB; a.nEnd = nEnd; a.nPix = nPix;
  // words per band of the LDS slice: nEnd * Q rounded up to an odd number of 16-byte pieces (the lanes of the staging store
  // then spread over 8 banks), or 0 for the table in global memory
  a.stride = (long long)nEnd * Q <= SCF_TAB_LDS ? 4 * (((nEnd * Q + 3) / 4) | 1) : 0;
  return 0;
}
