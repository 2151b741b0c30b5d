// What the continuum kernels share (DESIGN.md sections 4.22 and 4.23): rtx_continuum.hip adds the tabulated continuum to a
// block of optical depths, rtx_continuum_d.hip its derivatives in layer temperature and mixing ratio. Both form a point's
// stencil, weights and radiation term with the code below, so the mask max(0, .) applied in the one is the mask the other
// differentiates under, bit for bit.
#pragma once
#include "rtx_common.h"

#define CT_BLOCK 256
#define CT_PER 4                       // points per thread: one 16-byte access
#define CT_TILE (CT_BLOCK * CT_PER)    // consecutive points owned by a workgroup
#define CT_GROUP 4                     // components whose per-point stencils are held in registers at once
#define CT_C2 1.43877736830            // radiative_transfer.py:72 in cm K

struct __attribute__((aligned(8))) ContComp {
  double v0, dv, vend;  // vend = v0 + (n - 1) * dv, unfused: the last point that is inside
  int n, pad;
};

// tanh(x/2) = (1 - e) / (1 + e), e = exp(-x), one exponential; below x = 1/8 the difference 1 - e loses bits to
// cancellation and the odd series in h = x/2 (next term 62 h^9 / 2835 < 1e-12 h) takes over.
__device__ __forceinline__ float tanh_half_series(float x) {
  const float h = 0.5f * x, h2 = h * h;
  return h * fmaf(h2, fmaf(h2, fmaf(h2, -17.0f / 315.0f, 2.0f / 15.0f), -1.0f / 3.0f), 1.0f);
}

// nu tanh(c2 nu / (2T)) from x = c2 nu / T.
__device__ __forceinline__ float radiation_term(float nu, float x) {
  float th;
  if (x < 0.125f) {
    th = tanh_half_series(x);
  } else {
    const float e = __builtin_amdgcn_exp2f(-x * (float)LOG2E);
    th = (1.0f - e) * __builtin_amdgcn_rcpf(1.0f + e);
  }
  return nu * th;
}

// Stencil start and the four Lagrange weights of one point on one component's axis, from the point's fp64 wavenumber
// (nu - nu_j0 is formed in fp64, then rounded); a point outside the axis gets j0 = 0 and weights 0.
__device__ __forceinline__ int cont_stencil(const ContComp& cc, double nu, float (&L)[4]) {
  const bool in = nu >= cc.v0 && nu <= cc.vend;
  int jj = (int)floor((nu - cc.v0) / cc.dv) - 1;
  jj = !in ? 0 : jj < 0 ? 0 : jj > cc.n - 4 ? cc.n - 4 : jj;
  const double nj = __dadd_rn(cc.v0, __dmul_rn((double)jj, cc.dv));
  const float t = (float)((nu - nj) / cc.dv);
  const float t1 = t - 1.0f, t2 = t - 2.0f, t3 = t - 3.0f;
  L[0] = in ? -(1.0f / 6.0f) * (t1 * t2 * t3) : 0.0f;
  L[1] = in ? 0.5f * (t * t2 * t3) : 0.0f;
  L[2] = in ? -0.5f * (t * t1 * t3) : 0.0f;
  L[3] = in ? (1.0f / 6.0f) * (t * t1 * t2) : 0.0f;
  return jj;
}

// sum_k L_k a_k as both kernels chain it.
__device__ __forceinline__ float cont_stencil_sum(const float (&L)[4], float a0, float a1, float a2, float a3) {
  return fmaf(L[3], a3, fmaf(L[2], a2, fmaf(L[1], a1, L[0] * a0)));
}
