// fp64 complex arithmetic and the complex probability functions of hapi's line profiles (hum1_wei, misc/hapi.py:9833;
// cpf3, :9645), shared by the speed-dependent Voigt line-sum (rtx_sdvoigt.hip) and the line-profile functions
// (rtx_pcqsdhc.h, rtx_profiles.hip). Moved verbatim out of rtx_sdvoigt.hip. Mind the stated domains: fast_rcp, fast_sqrt
// and everything built on them (cinv, cdiv, cabs, csqrt_) are for arguments whose squares neither overflow nor go
// subnormal; code that takes arbitrary user parameters uses the library forms of rtx_pcqsdhc.h instead.
#pragma once
#ifndef RTX_CPLX_MATH_HOST  // tests/pcqsdhc_host_main.cpp compiles this arithmetic for the host and supplies what it names
#include "rtx_voigt_math.h"
#endif

struct cd {
  double r, i;
};
__device__ __forceinline__ cd cmul(cd a, cd b) { return {a.r * b.r - a.i * b.i, a.r * b.i + a.i * b.r}; }
__device__ __forceinline__ cd cadd(cd a, cd b) { return {a.r + b.r, a.i + b.i}; }
__device__ __forceinline__ cd csub(cd a, cd b) { return {a.r - b.r, a.i - b.i}; }
__device__ __forceinline__ cd cscale(cd a, double s) { return {a.r * s, a.i * s}; }
// Reciprocal and square root without the library's range handling: the arguments here are sums of squares of O(1e-6 .. 1e6)
// quantities -- never subnormal, never near overflow -- so v_rcp_f64 / v_rsq_f64 (2^-26) plus two Newton steps (<= 1 ulp, as in
// rtx_voigt_math.h: weideman_re) replace the IEEE division sequence (div_scale / div_fmas / div_fixup) and the scaled sqrt:
// ~8 instead of ~15 and ~30 instructions, four to six of them per profile evaluation in a kernel that is bound by fp64 issue.
__device__ __forceinline__ double fast_rcp(double d) {
  double r = __builtin_amdgcn_rcp(d);
  r = fma(fma(-d, r, 1.0), r, r);
  r = fma(fma(-d, r, 1.0), r, r);
  return r;
}
__device__ __forceinline__ double fast_sqrt(double s) {  // s >= 0
  const double y = __builtin_amdgcn_rsq(s);
  double g = s * y, h = 0.5 * y;
  double r = fma(-h, g, 0.5);
  g = fma(g, r, g);
  h = fma(h, r, h);
  r = fma(-h, g, 0.5);
  g = fma(g, r, g);
  h = fma(h, r, h);
  g = fma(fma(-g, g, s), h, g);
  return s > 0.0 ? g : 0.0;
}
__device__ __forceinline__ cd cinv(cd a) {
  const double d = fast_rcp(a.r * a.r + a.i * a.i);
  return {a.r * d, -a.i * d};
}
__device__ __forceinline__ cd cdiv(cd a, cd b) { return cmul(a, cinv(b)); }
// |a| without hypot's scaling (the arguments here are O(1e-6 .. 1e6): no overflow or underflow to guard against; the
// library hypot costs more than the rest of the far-wing evaluation, and the 1-ulp difference is far below the 1e-9 the
// parity tests hold this path to)
__device__ __forceinline__ double cabs(cd a) { return fast_sqrt(a.r * a.r + a.i * a.i); }
// principal square root (numpy.sqrt on complex128)
__device__ __forceinline__ cd csqrt_(cd z) {
  const double m = cabs(z);
  if (m == 0.0) return {0.0, z.i};
  if (z.r >= 0.0) {
    const double t = fast_sqrt(0.5 * (m + z.r));
    return {t, z.i * fast_rcp(2.0 * t)};
  }
  const double t = fast_sqrt(0.5 * (m - z.r));
  return {fabs(z.i) * fast_rcp(2.0 * t), copysign(t, z.i)};
}

// hum1_wei, misc/hapi.py:9833-9844: w(x + iy), Weideman's 24-term expansion where |x| + y < 15, else the one-term
// asymptote (1/sqrt(pi)) t / (1/2 + t^2), t = y - ix.
__device__ cd hum1_wei_c(double x, double y) {
  if (fabs(x) + y < 15.0) {
    const double L = W24_L;
    const cd d = {L + y, -x};  // L - i z, z = x + iy
    const cd n = {L - y, x};   // L + i z
    const cd Z = cdiv(n, d);
    cd p = {W24D[0], 0.0};
#pragma unroll
    for (int k = 1; k < 24; ++k) {
      p = cmul(p, Z);
      p.r += W24D[k];
    }
    const cd id = cinv(d);
    const cd w = cadd(cscale(cmul(p, cmul(id, id)), 2.0), cscale(id, INV_SQRT_PI));
    return w;
  }
  const cd t = {y, -x};
  cd den = cmul(t, t);
  den.r += 0.5;
  return cscale(cdiv(t, den), INV_SQRT_PI);
}

// Re hum1_wei for the branches that only need real parts (PART1, PART2, PART4: Re(Aterm) = sqrt(pi) cte (Re W1 - Re W2)):
// the real two-term recurrence of the Voigt line-sum's fp64 band (rtx_voigt_math.h: weideman_re, half the operations of
// the complex Horner form and two independent chains; within 1.5e-15 absolute of numpy.polyval). y >= 0 only.
__device__ __forceinline__ double hum1_wei_asym_re(double x, double y) {
  const cd t = {y, -x};
  cd den = cmul(t, t);
  den.r += 0.5;
  return cdiv(t, den).r * INV_SQRT_PI;
}
// Re w(z1) - Re w(z2); both Weideman evaluations in one straight-line block when both arguments are inside |x| + y < 15,
// so that their recurrences interleave
__device__ __forceinline__ double hum1_wei_re_diff(double x1, double y1, double x2, double y2) {
  const bool in1 = fabs(x1) + y1 < 15.0, in2 = fabs(x2) + y2 < 15.0;
  if (in1 && in2) return weideman_re<double>(x1, y1) - weideman_re<double>(x2, y2);
  const double w1 = in1 ? weideman_re<double>(x1, y1) : hum1_wei_asym_re(x1, y1);
  const double w2 = in2 ? weideman_re<double>(x2, y2) : hum1_wei_asym_re(x2, y2);
  return w1 - w2;
}

// cpf3, misc/hapi.py:9645-9670: 15-term asymptotic series
__device__ cd cpf3_c(double x, double y) {
  const cd zm1 = cinv(cd{x, y});
  const cd zm2 = cmul(zm1, zm1);
  cd zsum = {1.0, 0.0}, zterm = {1.0, 0.0};
#pragma unroll
  for (int k = 0; k < 15; ++k) {
    zterm = cscale(cmul(zterm, zm2), 0.5 + (double)k);
    zsum = cadd(zsum, zterm);
  }
  const cd izm1 = {-zm1.i, zm1.r};  // i * zm1
  return cscale(cmul(zsum, izm1), 0.564189583547756);
}
