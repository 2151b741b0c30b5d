// The complete pcqsdhc (partially-correlated quadratic-speed-dependent hard-collision, i.e. Hartmann-Tran) profile of
// misc/hapi.py:9850-10023 for ONE point, complex, in fp64: PART1 .. PART4 with Aterm and Bterm, and the common part
//   LS = (1/pi) A / (1 - (anuVC - eta (c0 - 1.5 c2)) A + eta c2 B),   eta complex.
// rtx_sdvoigt.hip: sdvoigt_profile is the slice Re(A)/pi of it for anuVC = eta = Shift2 = 0 on a line table's parameters; this
// one takes arbitrary user parameters (rtx_profile_eval / rtx_profile_sum), so
//   * every quantity is formed as the reference writes it, in its order of operations (c0t, c2t, X, Y, csqrtY all complex);
//   * each point is on its own: the value is what the reference returns for sg = array([s]) (its vector call assigns Bterm
//     whole-array in PART1 and mis-indexes its work arrays when the points of a call split between PARTs);
//   * PART3's far form takes PART3's own W (the reference reads an unbound WR1 there);
//   * divisions, square roots and moduli are the library's (IEEE division, sqrt, hypot; complex division by Smith's
//     algorithm, which is also NumPy's), not rtx_cplx_math.h's fast_rcp / fast_sqrt / cabs forms, whose domain -- squares
//     that neither overflow nor go subnormal, O(1e-6 .. 1e6) arguments -- user parameters and PART3 (|X| >= 1e15 |Y|) leave.
//     hum1_wei_c and cpf3_c are reused only where their domain holds: cpf3 on its shell 7 < |z| < 9, and the Weideman
//     branch (|x| + y < 15), whose two reciprocals are of |L - iz|^2. The region does not bound that above when y < 0
//     (x = 1e6, y = -1e6 is inside it), but the square only overflows beyond |z| ~ 1e154, where the reference's own
//     (L - iz)**2 overflows too; below it is small only at the expansion's own pole z = -iL;
//   * y = Re Z may be negative (Gam0 < 1.5 Gam2): no real-only shortcut is taken anywhere.
// Bterm is skipped when eta is exactly 0 (it is multiplied by eta c2); nothing else is dropped. Parameters are not
// validated: GamD = 0 or eta = 1 give what IEEE arithmetic gives, as in the reference.
// The profile is two out-of-line bodies, the per-line constants (ht_setup) and the per-point value (ht_point): inlined at
// several call sites the speed-dependent Voigt kernel was 162 KB of code against a 64 KB instruction cache.
#pragma once
#include "rtx_cplx_math.h"

// numpy's complex division (Smith's algorithm, npymath / the loops of umath): no |b|^2, so no overflow or underflow of it
__device__ __forceinline__ cd cdiv_lib(cd a, cd b) {
  if (fabs(b.r) >= fabs(b.i)) {
    const double rat = b.i / b.r, scl = 1.0 / (b.r + b.i * rat);
    return {(a.r + a.i * rat) * scl, (a.i - a.r * rat) * scl};
  }
  const double rat = b.r / b.i, scl = 1.0 / (b.i + b.r * rat);
  return {(a.r * rat + a.i) * scl, (a.i * rat - a.r) * scl};
}
__device__ __forceinline__ double cabs_lib(cd a) { return hypot(a.r, a.i); }
// principal square root as the C library forms it (numpy.sqrt on complex128)
__device__ __forceinline__ cd csqrt_lib(cd z) {
  const double d = hypot(z.r, z.i);
  if (d == 0.0) return {0.0, z.i};
  if (z.r > 0.0) {
    const double r = sqrt(0.5 * (d + z.r));
    return {r, 0.5 * (z.i / r)};
  }
  const double s = sqrt(0.5 * (d - z.r));
  return {fabs(0.5 * (z.i / s)), copysign(s, z.i)};
}
__device__ __forceinline__ cd one_minus_sq(cd z) {  // 1 - z**2
  const cd q = cmul(z, z);
  return {1.0 - q.r, -q.i};
}

// VARIABLES['CPF'] = hum1_wei (misc/hapi.py:9833-9846) for any argument, y < 0 included: Weideman's 24 terms inside
// |x| + y < 15, else the one-term asymptote (1/sqrt(pi)) t / (1/2 + t^2), t = y - ix, with the library division
__device__ __forceinline__ cd cpf_lib(double x, double y) {
  if (fabs(x) + y < 15.0) return hum1_wei_c(x, y);
  const cd t = {y, -x};
  cd den = cmul(t, t);
  den.r += 0.5;
  return cdiv_lib(cscale(t, INV_SQRT_PI), den);
}

// Per-line constants of pcqsdhc (:9900-9907, :9927-9928 and the factors of the common part :10022)
struct __attribute__((aligned(16))) HtLine {
  double sg0, cte;
  cd c0t, c2t;  // (1 - eta)(c0 - 1.5 c2) + anuVC, (1 - eta) c2
  cd Y, csqrtY; // 1 / (2 cte c2t)^2, (Gam2 - i Shift2) / (2 cte (1 - eta)(Gam2^2 + Shift2^2))
  cd k2;        // sqrt(pi) / (2 csqrtY)
  cd ka, kb;    // anuVC - eta (c0 - 1.5 c2), eta c2
  double absY;
  int part1;    // |c2t| == 0
  int need_b;   // eta != 0
};
#define HT_RPI 1.7724538509055159       // sqrt(pi)
#define HT_SQRT_LN2 0.8325546111576977  // sqrt(log(2.0)) as NumPy rounds it

// p[10]: sg0, GamD, Gam0, Gam2, Shift0, Shift2, anuVC, Re eta, Im eta, pad
__device__ __noinline__ void ht_setup(const double* __restrict__ p, HtLine* __restrict__ out) {
  HtLine L;
  L.sg0 = p[0];
  L.cte = HT_SQRT_LN2 / p[1];
  const double Gam2 = p[3], Shift2 = p[5], anuVC = p[6];
  const cd eta = {p[7], p[8]};
  const cd c0 = {p[2], p[4]}, c2 = {Gam2, Shift2};
  const cd ome = {1.0 - eta.r, -eta.i};
  const cd c02 = csub(c0, cscale(c2, 1.5));
  L.c0t = cmul(ome, c02);
  L.c0t.r += anuVC;
  L.c2t = cmul(ome, c2);
  const cd ec = cmul(eta, c02);
  L.ka = {anuVC - ec.r, -ec.i};
  L.kb = cmul(eta, c2);
  L.part1 = L.c2t.r == 0.0 && L.c2t.i == 0.0;
  L.need_b = eta.r != 0.0 || eta.i != 0.0;
  L.Y = L.csqrtY = L.k2 = {0.0, 0.0};
  L.absY = 0.0;
  if (!L.part1) {
    const cd t = cscale(L.c2t, 2.0 * L.cte);
    L.Y = cdiv_lib(cd{1.0, 0.0}, cmul(t, t));
    L.csqrtY = cdiv_lib(cd{Gam2, -Shift2}, cscale(cscale(ome, 2.0 * L.cte), Gam2 * Gam2 + Shift2 * Shift2));
    L.k2 = cdiv_lib(cd{HT_RPI, 0.0}, cscale(L.csqrtY, 2.0));
    L.absY = cabs_lib(L.Y);
  }
  *out = L;
}

// LS of pcqsdhc at wavenumber sg (complex: absorption and dispersion parts)
__device__ __noinline__ cd ht_point(const HtLine* __restrict__ Lp, const double sg) {
  const HtLine L = *Lp;
  const double rpi = HT_RPI, cte = L.cte, rc = rpi * cte;
  const cd num = {L.c0t.r, (L.sg0 - sg) + L.c0t.i};  // i (sg0 - sg) + c0t
  cd A, B = {0.0, 0.0};
  if (L.part1) {  // PART1 (:9910-9921)
    const cd Z1 = cscale(num, cte);
    const cd W = cpf_lib(-Z1.i, Z1.r);
    A = cscale(W, rc);
    if (L.need_b) {
      if (cabs_lib(Z1) <= 4.0e3) {
        const cd t = cadd(cmul(one_minus_sq(Z1), W), cscale(Z1, 1.0 / rpi));
        B = cscale(t, rc);
      } else {
        const cd Z3 = cmul(cmul(Z1, Z1), Z1);
        const cd t = csub(cadd(cscale(W, rpi), cdiv_lib(cd{0.5, 0.0}, Z1)), cdiv_lib(cd{0.75, 0.0}, Z3));
        B = cscale(t, cte);
      }
    }
  } else {
    const cd X = cdiv_lib(num, L.c2t);
    const double aX = cabs_lib(X);
    const bool part2 = aX <= 3.0e-8 * L.absY;
    if (!part2 && L.absY <= 1.0e-15 * aX) {  // PART3 (:9996-10019)
      const cd sXY = csqrt_lib(cadd(X, L.Y)), sX = csqrt_lib(X);
      const cd ic2t = cdiv_lib(cd{1.0, 0.0}, L.c2t);
      cd g;
      const bool near = cabs_lib(sX) <= 4.0e3;
      if (near) {
        const cd t = cmul(sX, cpf_lib(-sX.i, sX.r));
        g = {1.0 / rpi - t.r, -t.i};
        A = cmul(cdiv_lib(cd{2.0 * rpi, 0.0}, L.c2t), g);
      } else {
        g = csub(cdiv_lib(cd{1.0, 0.0}, X), cdiv_lib(cd{1.5, 0.0}, cmul(X, X)));
        A = cmul(ic2t, g);
      }
      if (L.need_b) {
        const cd W3 = cpf_lib(-sXY.i, sXY.r);
        const cd u = {1.0 - X.r - 2.0 * L.Y.r, -X.i - 2.0 * L.Y.i};  // 1 - X - 2 Y
        const cd t1 = cmul(near ? cscale(u, 2.0 * rpi) : u, g);
        const cd t2 = cmul(cscale(sXY, 2.0 * rpi), W3);
        B = cmul(ic2t, cadd(cd{-1.0 + t1.r, t1.i}, t2));
      }
    } else {
      cd Z1, Z2, W1, W2;
      if (part2) {  // PART2 (:9978-9993)
        Z1 = cscale(num, cte);
        Z2 = cadd(csqrt_lib(cadd(X, L.Y)), L.csqrtY);
        W1 = cpf_lib(-Z1.i, Z1.r);
        W2 = cpf_lib(-Z2.i, Z2.r);
      } else {  // PART4 (:9935-9975)
        Z1 = csub(csqrt_lib(cadd(X, L.Y)), L.csqrtY);
        Z2 = cadd(Z1, cscale(L.csqrtY, 2.0));
        const double x1 = -Z1.i, y1 = Z1.r, x2 = -Z2.i, y2 = Z2.r;
        const double S1 = sqrt(x1 * x1 + y1 * y1), S2 = sqrt(x2 * x2 + y2 * y2);
        // cpf3 in the shell around |Z| = 8 where the two arguments straddle it (:9953)
        if (fabs(S1 - S2) <= 1.0 && fmax(S1, S2) > 8.0 && fmin(S1, S2) <= 8.0) {
          W1 = cpf3_c(x1, y1);
          W2 = cpf3_c(x2, y2);
        } else {
          W1 = cpf_lib(x1, y1);
          W2 = cpf_lib(x2, y2);
        }
      }
      A = cscale(csub(W1, W2), rc);
      if (L.need_b) {
        const cd t1 = cmul(cmul(L.k2, one_minus_sq(Z1)), W1);
        const cd t2 = cmul(cmul(L.k2, one_minus_sq(Z2)), W2);
        B = cdiv_lib(csub(cd{-1.0 + t1.r, t1.i}, t2), L.c2t);
      }
    }
  }
  // common part (:10022)
  const cd kA = cmul(L.ka, A);
  cd den = {1.0 - kA.r, -kA.i};
  if (L.need_b) den = cadd(den, cmul(L.kb, B));
  return cscale(cdiv_lib(A, den), 1.0 / M_PI);
}
