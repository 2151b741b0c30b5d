// hapi's line-profile functions with explicit per-line parameters (misc/hapi.py:9850-10160: pcqsdhc / PROFILE_HT and its
// limits, PROFILE_LORENTZ, PROFILE_DOPPLER) and the complex probability functions under them (hum1_wei :9833, cpf3 :9645):
// no line table, no environment, no windows -- every line reaches every point. fp64 throughout, complex output (the
// imaginary part is the dispersion shape that first-order line mixing needs). The profile itself is rtx_pcqsdhc.h;
// DESIGN.md section 4.14.
#include "rtx_common.h"

#include "rtx_voigt_math.h"
#include "rtx_pcqsdhc.h"

#define PF_BLOCK 256
#define PF_NPAR 10        // doubles per line: sg0, GamD, Gam0, Gam2, Shift0, Shift2, anuVC, Re eta, Im eta, pad
#define PF_MAX_Y 65535    // lines per launch of the evaluation kernel (grid.y)
#define PF_CHUNK 128      // lines whose constants one workgroup of the sum kernel holds in LDS (128 x 144 B = 18 KiB)
// hapi's own rounded constants (misc/hapi.py:89-90)
#define HAPI_SQRT_LN2_DIV_SQRT_PI 0.469718639319144059835
#define HAPI_LN2 0.6931471805599

// ---- every line at every point: line = blockIdx.y (its parameters are wave-uniform), point = blockIdx.x * 256 + threadIdx.x --
__global__ __launch_bounds__(PF_BLOCK) void profile_eval_kernel(int kind, const double* __restrict__ params, const double* __restrict__ sg,
                                                                long long n, double* __restrict__ out_re, double* __restrict__ out_im,
                                                                long long ld) {
  __shared__ HtLine s_line;
  const double* __restrict__ p = params + (size_t)blockIdx.y * PF_NPAR;
  if (kind == RTX_LS_PCQSDHC) {  // the line's constants once per workgroup
    if (threadIdx.x == 0) ht_setup(p, &s_line);
    __syncthreads();
  }
  const long long i = (long long)blockIdx.x * PF_BLOCK + threadIdx.x;
  if (i >= n) return;
  const double s = sg[i];
  cd v = {0.0, 0.0};
  if (kind == RTX_LS_PCQSDHC) {
    v = ht_point(&s_line, s);
  } else if (kind == RTX_LS_LORENTZ) {  // Gam0 / (pi (Gam0^2 + (sg - sg0)^2)), :10150
    const double sg0 = p[0], Gam0 = p[2], d = s - sg0;
    v.r = Gam0 / (M_PI * (Gam0 * Gam0 + d * d));
  } else {  // cSqrtLn2divSqrtPi exp(-cLn2 ((sg - sg0) / GamD)^2) / GamD, :10160
    const double sg0 = p[0], GamD = p[1], t = (s - sg0) / GamD;
    v.r = HAPI_SQRT_LN2_DIV_SQRT_PI * exp(-HAPI_LN2 * (t * t)) / GamD;
  }
  const size_t o = (size_t)blockIdx.y * (size_t)ld + (size_t)i;
  out_re[o] = v.r;
  if (out_im) out_im[o] = v.i;
}

// ---- the model spectrum of a fit: out[i] = sum_l w_re[l] Re LS_l(sg_i) + w_im[l] Im LS_l(sg_i) ---------------------------------
// One thread per point, the lines in index order with one association (acc = acc + (w_re Re + w_im Im)): a point's value
// does not depend on the launch shape and is bit-reproducible. The constants of PF_CHUNK lines at a time are formed by the
// workgroup's first PF_CHUNK threads (one line each) and read by all of them from LDS.
__global__ __launch_bounds__(PF_BLOCK) void profile_sum_kernel(long long n_lines, const double* __restrict__ params,
                                                               const double* __restrict__ w_re, const double* __restrict__ w_im,
                                                               const double* __restrict__ sg, long long n, double* __restrict__ out) {
  __shared__ HtLine s_line[PF_CHUNK];
  const long long i = (long long)blockIdx.x * PF_BLOCK + threadIdx.x;
  const double s = i < n ? sg[i] : 0.0;
  double acc = 0.0;
  for (long long base = 0; base < n_lines; base += PF_CHUNK) {
    const int m = (int)(n_lines - base < PF_CHUNK ? n_lines - base : PF_CHUNK);
    __syncthreads();  // the previous chunk is no longer read
    if ((int)threadIdx.x < m) ht_setup(params + (size_t)(base + threadIdx.x) * PF_NPAR, &s_line[threadIdx.x]);
    __syncthreads();
    if (i < n) {
      for (int j = 0; j < m; ++j) {
        const cd v = ht_point(&s_line[j], s);
        double t = w_re[base + j] * v.r;
        if (w_im) t = t + w_im[base + j] * v.i;
        acc = acc + t;
      }
    }
  }
  if (i < n) out[i] = acc;
}

// ---- hum1_wei / cpf3 elementwise --------------------------------------------------------------------------------------
__global__ __launch_bounds__(PF_BLOCK) void cpf_eval_kernel(int kind, const double* __restrict__ x, const double* __restrict__ y, long long n,
                                                            double* __restrict__ out_re, double* __restrict__ out_im) {
  const long long i = (long long)blockIdx.x * PF_BLOCK + threadIdx.x;
  if (i >= n) return;
  const cd w = kind == RTX_CPF_HUM1_WEI ? cpf_lib(x[i], y[i]) : cpf3_c(x[i], y[i]);
  out_re[i] = w.r;
  if (out_im) out_im[i] = w.i;
}

static int pf_blocks(int64_t n, unsigned* out) {
  const int64_t b = (n + PF_BLOCK - 1) / PF_BLOCK;
  if (b > 2147483647LL) RTX_FAIL("n=%lld points: more than 2^31 - 1 workgroups", (long long)n);
  *out = (unsigned)b;
  return 0;
}

extern "C" int rtx_profile_eval(int kind, int64_t n_lines, const double* params, const double* sg, int64_t n, double* out_re,
                                double* out_im, int64_t ld, void* stream) {
  if (!params || !sg || !out_re) RTX_FAIL("a required pointer is NULL (params, sg, out_re)");
  if (kind < RTX_LS_PCQSDHC || kind > RTX_LS_DOPPLER) RTX_FAIL("kind=%d", kind);
  if (n_lines < 0 || n < 0) RTX_FAIL("n_lines=%lld n=%lld", (long long)n_lines, (long long)n);
  if (ld < n) RTX_FAIL("ld=%lld smaller than n=%lld", (long long)ld, (long long)n);
  if (n_lines == 0 || n == 0) return 0;  // nothing to do: no launch
  unsigned bx;
  if (pf_blocks(n, &bx)) return 1;
  for (int64_t l0 = 0; l0 < n_lines; l0 += PF_MAX_Y) {
    const int64_t nl = n_lines - l0 < PF_MAX_Y ? n_lines - l0 : PF_MAX_Y;
    hipLaunchKernelGGL(profile_eval_kernel, dim3(bx, (unsigned)nl), dim3(PF_BLOCK), 0, (hipStream_t)stream, kind,
                       params + (size_t)l0 * PF_NPAR, sg, (long long)n, out_re + (size_t)l0 * (size_t)ld,
                       out_im ? out_im + (size_t)l0 * (size_t)ld : nullptr, (long long)ld);
    RTX_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int rtx_profile_sum(int64_t n_lines, const double* params, const double* w_re, const double* w_im, const double* sg,
                               int64_t n, double* out, void* stream) {
  if (!params || !w_re || !sg || !out) RTX_FAIL("a required pointer is NULL (params, w_re, sg, out)");
  if (n_lines < 0 || n < 0) RTX_FAIL("n_lines=%lld n=%lld", (long long)n_lines, (long long)n);
  if (n_lines == 0 || n == 0) return 0;  // nothing to do: no launch (out is not written)
  unsigned bx;
  if (pf_blocks(n, &bx)) return 1;
  hipLaunchKernelGGL(profile_sum_kernel, dim3(bx), dim3(PF_BLOCK), 0, (hipStream_t)stream, (long long)n_lines, params, w_re, w_im, sg,
                     (long long)n, out);
  RTX_LAUNCH_CHECK();
  return 0;
}

extern "C" int rtx_cpf_eval(int kind, const double* x, const double* y, int64_t n, double* out_re, double* out_im, void* stream) {
  if (!x || !y || !out_re) RTX_FAIL("a required pointer is NULL (x, y, out_re)");
  if (kind != RTX_CPF_HUM1_WEI && kind != RTX_CPF_CPF3) RTX_FAIL("kind=%d", kind);
  if (n < 0) RTX_FAIL("n=%lld", (long long)n);
  if (n == 0) return 0;
  unsigned bx;
  if (pf_blocks(n, &bx)) return 1;
  hipLaunchKernelGGL(cpf_eval_kernel, dim3(bx), dim3(PF_BLOCK), 0, (hipStream_t)stream, kind, x, y, (long long)n, out_re, out_im);
  RTX_LAUNCH_CHECK();
  return 0;
}
