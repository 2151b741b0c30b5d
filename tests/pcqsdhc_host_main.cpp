// The device arithmetic of the line-profile functions (radtxfr_amd/csrc/rtx_pcqsdhc.h over rtx_cplx_math.h) compiled for the
// HOST, so that every branch of the profile can be compared with the reference's values without a GPU
// (tests/test_profiles_host.py builds this with -I radtxfr_amd/csrc; RTX_CPLX_MATH_HOST keeps rtx_cplx_math.h from including
// the HIP headers). The device qualifiers are defined away; the two hardware approximations that fast_rcp / fast_sqrt refine
// by Newton steps are stood in for by the exact quotient and root, which those steps converge to within an ulp. Compile with
// -ffp-contract=off, as the library is.
// stdin: records "0 p[0..9] n sg[0..n)" (pcqsdhc), "1 n (x y)*n" (hum1_wei), "2 n (x y)*n" (cpf3); stdout: "re im" per point.
#include <math.h>
#include <stdio.h>
#define RTX_CPLX_MATH_HOST
#define __device__
#define __forceinline__ inline
#define __noinline__
#define INV_SQRT_PI 0.56418958354775628
#include "w24_coeffs.inc"
static inline double __builtin_amdgcn_rcp(double d) { return 1.0 / d; }
static inline double __builtin_amdgcn_rsq(double d) { return 1.0 / sqrt(d); }
template <typename F>
F weideman_re(F, F);  // the real-only recurrence of rtx_voigt_math.h: named by the SDVoigt shortcuts, never called here
#include "rtx_pcqsdhc.h"

int main() {
  int mode, n;
  while (scanf("%d", &mode) == 1) {
    if (mode == 0) {
      double p[10];
      for (int i = 0; i < 10; ++i)
        if (scanf("%lf", &p[i]) != 1) return 2;
      if (scanf("%d", &n) != 1) return 2;
      HtLine L;
      ht_setup(p, &L);
      for (int i = 0; i < n; ++i) {
        double s;
        if (scanf("%lf", &s) != 1) return 2;
        const cd v = ht_point(&L, s);
        printf("%.17g %.17g\n", v.r, v.i);
      }
    } else {
      if (scanf("%d", &n) != 1) return 2;
      for (int i = 0; i < n; ++i) {
        double x, y;
        if (scanf("%lf %lf", &x, &y) != 2) return 2;
        const cd v = mode == 1 ? cpf_lib(x, y) : cpf3_c(x, y);
        printf("%.17g %.17g\n", v.r, v.i);
      }
    }
  }
  return 0;
}
