// What rtx_tud.hip and rtx_tud_jac.hip share: the thin-layer emissivity on the device, and on the host the angle
// quadrature and the per-layer Planck constants, each formed in one place so that the Jacobian
// differentiates exactly the numbers the TUD kernels integrate.
#pragma once
#include <vector>

#include "rtx_common.h"

// 1 - exp(-OD*sec) = 1 - 2^y (y = OD*c <= 0), accurate to ~1e-7 RELATIVE also when it is tiny.
// A layer's emissivity (1 - t) is what weights its Planck radiance in L <- t L + (1 - t) B; forming it as 1 - fl(t)
// from v_exp_f32 loses everything once t is within a few ulp of 1 (an optically thin layer: the LWIR window),
// and the error of the accumulated radiance then reaches 1e-5..1e-4 of a thin path's radiance. So:
//   |y| <  1/16 : 1 - 2^y = -y*ln2*(1 + z/2 + z^2/6 + z^3/24), z = y ln2            (truncation 2.9e-8)
//   |y| >= 1/16 : 1 - v_exp_f32(y)                                                    (relative error <= 1.4e-6)
// (round 1: degree 5 below 1/8, 7e-9 / 7e-7; one operation more per stream and layer)
#ifndef TUD_THIN_Y
#define TUD_THIN_Y 0.0625f
#endif
constexpr float EM_Q1 = 6.9314718056e-1f, EM_Q2 = 2.4022650696e-1f, EM_Q3 = 5.5504108665e-2f,
                EM_Q4 = 9.6181291076e-3f;  // ln2, ln2^2/2, ln2^3/6, ln2^4/24
__device__ __forceinline__ float em_thin(float y) {  // valid for -TUD_THIN_Y < y <= 0
  const float q = fmaf(fmaf(fmaf(EM_Q4, y, EM_Q3), y, EM_Q2), y, EM_Q1);
  return -y * q;
}
__device__ __forceinline__ float emissivity(float y) {  // any y <= 0
  return (y > -TUD_THIN_Y) ? em_thin(y) : 1.0f - __builtin_amdgcn_exp2f(y);
}

// ---- host ---------------------------------------------------------------------------------------------
// angles = linspace(0, pi/2, nA, endpoint=False) (radiative_transfer.py:368); weights cos*sin (:387) and their sum.
// theta = 0 is entry 0 and has weight exactly 0 (sin 0 = 0): callers that skip it start at 1.
struct TudQuadrature {
  std::vector<double> th, w;
  double wsum;
};
static inline TudQuadrature tud_quadrature(int n_angle) {
  TudQuadrature q;
  q.wsum = 0.0;
  const double dth = (M_PI / 2.0) / (double)n_angle;  // np.linspace step
  for (int ii = 0; ii < n_angle; ++ii) {
    q.th.push_back((double)ii * dth);
    q.w.push_back(cos(q.th[ii]) * sin(q.th[ii]));
    q.wsum += q.w[ii];
  }
  return q;
}

// 100 c2 log2(e) / T: x times it is the log2 of the Planck exponential (planck_f32)
static inline double c2l2e_over(double T) { return 100.0 * RT_C2 * LOG2E / T; }
static inline int tud_layer_consts(const double* T_h, int n_layers, double* c2l2e_over_T) {
  for (int k = 0; k < n_layers; ++k) {
    if (!(T_h[k] > 0.0)) RTX_FAIL("layer %d temperature %g", k, T_h[k]);
    c2l2e_over_T[k] = c2l2e_over(T_h[k]);
  }
  return 0;
}
