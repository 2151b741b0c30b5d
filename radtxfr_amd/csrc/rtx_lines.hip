// Line table upload + the fp64 per-(line,layer) prologue kernel.
//
// Replaces the per-line environment block of hapi.absorptionCoefficient_Voigt
// (reference misc/hapi.py:11068-11134) -- S(T), GammaD, Gamma0, Shift0, OmegaWingF and the two
// bisect() window bounds -- for all lines x all layers in one launch. fp64 throughout, operations
// in the reference's order, so the hard wing cutoff lands on the same grid points.
#include <math.h>
#include <stdarg.h>
#include <string.h>

#include "rtx_common.h"

// ---- error text ------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void rtx_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* rtx_last_error(void) { return g_err; }
extern "C" int rtx_version(void) { return RTX_VERSION; }
extern "C" int rtx_device_info(char* name_h, int len, int* n_cu_h) {
  int dev;
  RTX_HIP(hipGetDevice(&dev));
  hipDeviceProp_t p;
  RTX_HIP(hipGetDeviceProperties(&p, dev));
  if (name_h && len > 0) snprintf(name_h, len, "%s (%s)", p.name, p.gcnArchName);
  if (n_cu_h) *n_cu_h = p.multiProcessorCount;
  return 0;
}

int rtx_check_grid(const rtx_grid* g) {
  if (!g) RTX_FAIL("grid is NULL");
  if (g->n_total < 2) RTX_FAIL("grid needs at least 2 points (n_total=%lld)", (long long)g->n_total);
  if (!(g->step > 0.0)) RTX_FAIL("grid step must be > 0 (ascending axis)");
  if (g->offset < 0 || g->n < 0 || g->offset + g->n > g->n_total)
    RTX_FAIL("grid shard [%lld,+%lld) outside [0,%lld)", (long long)g->offset, (long long)g->n, (long long)g->n_total);
  if (g->n_total > 2000000000LL) RTX_FAIL("grid too long for 32-bit point indices");
  return 0;
}

// ---- device memory (rtx_devmem.h) -----------------------------------------------------------------
int rtx_dev_alloc(void** p, size_t bytes) {
  *p = nullptr;
  const hipError_t e = hipMalloc(p, bytes);
  if (e == hipSuccess) return 0;
  *p = nullptr;
  RTX_FAIL("device allocation of %zu bytes -> %s", bytes, hipGetErrorString(e));
}
void rtx_dev_free(void* p) {
  if (p) (void)hipFree(p);
}
int rtx_dev_h2d(void* d, const void* h, size_t bytes) {
  RTX_HIP(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));
  return 0;
}
int rtx_dev_current(int* dev) {
  RTX_HIP(hipGetDevice(dev));
  return 0;
}

// ---- line table ------------------------------------------------------------------------------------
// A column of n doubles (one element for an empty table, so that the pointer is never NULL); an optional column that is
// absent stays empty.
static int upload(DevBuf<double>& dst, const double* src_h, long long n, bool required) {
  if (!src_h && !required) return 0;
  if (dst.reserve((size_t)(n > 0 ? n : 1))) return 1;
  return n > 0 ? rtx_dev_h2d(dst.get(), src_h, sizeof(double) * (size_t)n) : 0;
}

extern "C" int rtx_lines_free(rtx_lines* L) {
  delete L;
  return 0;
}

int rtx_lines_fill_zn(rtx_lines* L);
extern "C" int rtx_lines_create(int64_t n, int n_species, const double* nu_h, const double* sw_h, const double* elower_h,
                                const double* gamma_air_h, const double* gamma_self_h, const double* n_air_h,
                                const double* n_self_h, const double* delta_air_h, const double* deltap_air_h,
                                const double* delta_self_h, const int32_t* species_h, rtx_lines** out) {
  if (!out) RTX_FAIL("out is NULL");
  *out = nullptr;
  if (n < 0 || n > 2000000000LL) RTX_FAIL("bad line count %lld", (long long)n);
  if (n_species < 1 || n_species > 4096) RTX_FAIL("n_species must be in [1,4096], got %d", n_species);
  if (n > 0 && (!nu_h || !sw_h || !elower_h || !gamma_air_h || !gamma_self_h || !n_air_h || !delta_air_h || !species_h))
    RTX_FAIL("a required line-table column is NULL");
  for (int64_t i = 0; i < n; ++i) {
    if (i > 0 && nu_h[i] < nu_h[i - 1]) RTX_FAIL("line table must be sorted by nu (row %lld)", (long long)i);
    if (species_h[i] < 0 || species_h[i] >= n_species) RTX_FAIL("species index out of range at row %lld", (long long)i);
  }
  rtx_lines* L = new rtx_lines();
  L->n = n;
  L->n_species = n_species;
  if (upload(L->nu, nu_h, n, true) || upload(L->sw, sw_h, n, true) || upload(L->elower, elower_h, n, true) ||
      upload(L->gamma_air, gamma_air_h, n, true) || upload(L->gamma_self, gamma_self_h, n, true) ||
      upload(L->n_air, n_air_h, n, true) || upload(L->n_self, n_self_h, n, false) || upload(L->delta_air, delta_air_h, n, true) ||
      upload(L->deltap_air, deltap_air_h, n, false) || upload(L->delta_self, delta_self_h, n, false) ||
      L->species.reserve((size_t)(n > 0 ? n : 1)) || (n > 0 && rtx_dev_h2d(L->species.get(), species_h, sizeof(int) * (size_t)n)) ||
      rtx_lines_fill_zn(L)) {
    delete L;
    return 1;
  }
  L->nu_host.assign(nu_h, nu_h + n);
  for (int64_t i = 0; i < n; ++i) {
    L->ga_max = fmax(L->ga_max, fabs(gamma_air_h[i]));
    L->gs_max = fmax(L->gs_max, fabs(gamma_self_h[i]));
    const double na = n_air_h[i], ns = (n_self_h && n_self_h[i] != 0.0) ? n_self_h[i] : na;
    L->n_lo = fmin(L->n_lo, fmin(na, ns));
    L->n_hi = fmax(L->n_hi, fmax(na, ns));
    L->na_lo = fmin(L->na_lo, na); L->na_hi = fmax(L->na_hi, na);
    L->ns_lo = fmin(L->ns_lo, ns); L->ns_hi = fmax(L->ns_hi, ns);
  }
  *out = L;
  return 0;
}
extern "C" int64_t rtx_lines_count(const rtx_lines* L) { return L ? L->n : -1; }

// An optional column: replaces the previous one; NULL (or an empty table) leaves none.
static int set_optional(DevBuf<double>& dst, const double* src_h, long long n) {
  dst.reset();
  return src_h && n > 0 ? dst.upload(src_h, (size_t)n) : 0;
}

extern "C" int rtx_lines_set_sd(rtx_lines* L, const double* sd_air_h, const double* sd_self_h) {
  if (!L) RTX_FAIL("lines is NULL");
  return set_optional(L->sd_air, sd_air_h, L->n) || set_optional(L->sd_self, sd_self_h, L->n);
}

extern "C" int rtx_lines_set_deltap_self(rtx_lines* L, const double* deltap_self_h) {
  if (!L) RTX_FAIL("lines is NULL");
  return set_optional(L->deltap_self, deltap_self_h, L->n);
}

// Extra broadener column sets (gamma_<sp>, n_<sp>, delta_<sp>, deltap_<sp>, SD_<sp> of misc/hapi.py:11090-11128, 10860-10890):
// replaces the table's previous set. Every device column is filled, the reference's fallbacks applied here once: an absent
// gamma / delta / deltap / SD column is 0, an absent n column is n_air (a foreign n of 0 stays 0). The new set is built
// aside and taken over whole: a failure leaves the table with no extra set.
extern "C" int rtx_lines_set_broadeners(rtx_lines* L, int n_extra, const double* const* gamma_h, const double* const* n_h,
                                        const double* const* delta_h, const double* const* deltap_h, const double* const* sd_h) {
  if (!L) RTX_FAIL("lines is NULL");
  if (n_extra < 0 || n_extra > RTX_MAX_BROADENERS) RTX_FAIL("n_extra=%d outside [0,%d]", n_extra, RTX_MAX_BROADENERS);
  DevBuf<double>* dst[5] = {&L->x_gamma, &L->x_n, &L->x_delta, &L->x_deltap, &L->x_sd};
  for (DevBuf<double>* d : dst) d->reset();
  L->x_gmax.clear(); L->x_nlo.clear(); L->x_nhi.clear();
  L->n_extra = 0;
  if (n_extra == 0) return 0;
  const size_t n = (size_t)L->n, cnt = (size_t)n_extra * (n > 0 ? n : 1);
  const double* const* src[5] = {gamma_h, n_h, delta_h, deltap_h, sd_h};
  DevBuf<double> cols[5];
  for (int c = 0; c < 5; ++c) {
    if (cols[c].reserve(cnt)) return 1;
    for (int j = 0; j < n_extra && n > 0; ++j) {
      double* col = cols[c].get() + (size_t)j * n;
      const double* h = src[c] ? src[c][j] : nullptr;
      if (h) { if (rtx_dev_h2d(col, h, n * sizeof(double))) return 1; }
      else if (c == 1) RTX_HIP(hipMemcpy(col, L->n_air.get(), n * sizeof(double), hipMemcpyDeviceToDevice));
      else RTX_HIP(hipMemset(col, 0, n * sizeof(double)));
    }
  }
  std::vector<double> gmax(n_extra), nlo(n_extra), nhi(n_extra);
  for (int j = 0; j < n_extra; ++j) {
    const double* g = gamma_h ? gamma_h[j] : nullptr;
    const double* nn = n_h ? n_h[j] : nullptr;
    double gm = 0.0, lo = L->na_lo, hi = L->na_hi;
    if (nn) { lo = 1e300; hi = -1e300; }
    for (size_t i = 0; i < n; ++i) {
      if (g) gm = fmax(gm, fabs(g[i]));
      if (nn) { lo = fmin(lo, nn[i]); hi = fmax(hi, nn[i]); }
    }
    gmax[j] = gm; nlo[j] = lo; nhi[j] = hi;
  }
  for (int c = 0; c < 5; ++c) *dst[c] = std::move(cols[c]);
  L->x_gmax = std::move(gmax); L->x_nlo = std::move(nlo); L->x_nhi = std::move(nhi);
  L->n_extra = n_extra;
  return 0;
}

// ---- prep object -------------------------------------------------------------------------------------
extern "C" int rtx_prep_free(rtx_prep* P) {
  delete P;
  return 0;
}

extern "C" int rtx_voigt_tile_points(void);

extern "C" int rtx_prep_create(const rtx_lines* lines, int max_layers, int64_t max_points, rtx_prep** out) {
  if (!out) RTX_FAIL("out is NULL");
  *out = nullptr;
  if (!lines) RTX_FAIL("lines is NULL");
  if (max_layers < 1 || max_layers > 4096) RTX_FAIL("max_layers must be in [1,4096]");
  if (max_points < 1 || max_points > 2000000000LL) RTX_FAIL("max_points must be in [1,2e9]");
  rtx_prep* P = new rtx_prep();
  P->n_lines = lines->n;
  P->max_layers = max_layers;
  const size_t n1 = (size_t)(lines->n > 0 ? lines->n : 1), nrec = n1 * (size_t)max_layers;
  const int tile = rtx_voigt_tile_points();
  P->max_tiles = (max_points + tile - 1) / tile;
  if (P->rec.reserve(nrec) || P->rec64.reserve(nrec) || P->ic.reserve(n1) || P->win.reserve(nrec) ||
      P->maxhw.reserve(2 * (size_t)max_layers + 1) ||
      P->env.reserve((size_t)max_layers * (2 + 2 * (size_t)lines->n_species) + (size_t)lines->n_species) ||
      P->ranges.reserve((size_t)P->max_tiles * (size_t)max_layers)) {
    delete P;
    return 1;
  }
  P->smally = P->maxhw.get() + max_layers;
  P->n_items = P->maxhw.get() + 2 * max_layers;
  *out = P;
  return 0;
}

// ---- prologue kernel --------------------------------------------------------------------------------
// hapi constants (misc/hapi.py:84-92, :10171, :11085)
#define H_CBOLTS 1.380648813e-16
#define H_CC 2.99792458e10
#define H_CMASSMOL 1.66053873e-27
#define H_C2 1.4388028496642257
#define H_TREF 296.0
#ifndef RTX_PREP_ABLATE
#define RTX_PREP_ABLATE 0
#endif
#define RTX_ENV_MAX 416  /* doubles of per-layer tables carried in the prologue's kernel arguments (3.3 KB of the 4 KB) */
#define RTX_MIX_MAX 8    /* diluents per mixed prologue (include/radtxfr_hip.h: RTX_MAX_DILUENTS) */
static_assert(RTX_MIX_MAX == RTX_MAX_DILUENTS, "kernel-argument diluent slots");

// The reference-temperature half of S(T) (misc/hapi.py:10171-10172) depends on the line alone: formed once per table, by the
// same expression the prologue used to evaluate per (line, layer) -- two of its four fp64 exponentials and two divisions.
__global__ __launch_bounds__(256) void lines_zn_kernel(const double* __restrict__ nu, const double* __restrict__ elower, double* __restrict__ zn,
                                                       long long n) {
  const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (l < n) zn[l] = exp(-H_C2 * elower[l] / H_TREF) * (1.0 - exp(-H_C2 * nu[l] / H_TREF));
}
int rtx_lines_fill_zn(rtx_lines* L) {
  if (L->n == 0) return 0;
  if (L->zn.reserve((size_t)L->n)) return 1;
  hipLaunchKernelGGL(lines_zn_kernel, dim3((unsigned)((L->n + 255) / 256)), dim3(256), 0, 0, L->nu.get(), L->elower.get(), L->zn.get(),
                     (long long)L->n);
  RTX_LAUNCH_CHECK();
  RTX_HIP(hipDeviceSynchronize());
  return 0;
}

struct PrepArgs {
  const double *nu, *sw, *elower, *gamma_air, *gamma_self, *n_air, *n_self, *delta_air, *deltap_air, *delta_self;
  const double *sd_air, *sd_self, *deltap_self;
  const double* zn;
  LineRecSD* recsd;
  const int* species;
  long long n_lines;
  int n_layers, n_species;
  const double *T, *p, *qratio, *weight, *mass;  // the small per-layer tables: device copies, or offsets into env[] (ENV_ARGS)
  double env[RTX_ENV_MAX];                       // T | p | qratio | weight | mass packed, when they fit (no H2D copy at all)
  double dil_air, dil_self, omega_wing, omega_wing_hw, thresh, scale;
  int profile;  // RTX_PROFILE_VOIGT / _LORENTZ / _DOPPLER
  GridDev g;
  const double* X;  // explicit axis (line_prep_axis_kernel): device copy, X[nx]
  long long nx;
  const double* Twin;  // line_prep_kernel<., true>: per-layer temperature of the windows (device copy, rtx_line_prep_window)
  LineRec* rec;
  LineRec64* rec64;
  int* ic;
  int2* win;
  int* maxhw;
  int* smally;
  // mixed prologue (MIX = true: rtx_line_prep_mix / _axis_mix): diluent d takes column set dil_idx[d] (0 air, 1 self, 2 + j
  // extra set j) with fraction frac[(d*n_species + species)*n_layers + layer] (device copy); x_* = the extra sets [n_extra][n]
  int n_dil;
  int dil_idx[RTX_MIX_MAX];
  const double* frac;
  const double *x_gamma, *x_n, *x_delta, *x_deltap, *x_sd;
};
static_assert(sizeof(PrepArgs) <= 4096, "the prologue's kernel arguments must stay within 4 KB");

// The per-layer tables (T, p, qratio, weight, mass: 324 doubles for 4 species x 32 layers) travel in the kernel arguments
// when they fit: the prologue then needs no host-to-device copy, which was 5 hipMemcpyAsync calls (~10 us of host time
// each) per atmosphere. Larger sets go through the prep object's device buffer as before.
// bisect.bisect (= bisect_right) of value v on the FULL grid: number of grid points <= v.
__device__ long long grid_bisect_right(const GridDev& g, double v) {
  double t = (v - g.xmin) / g.step;
  long long k;
  if (!(t > -1.0)) k = 0;
  else if (t >= (double)g.n_total) k = g.n_total;
  else k = (long long)floor(t) + 1;
  if (k < 0) k = 0;
  if (k > g.n_total) k = g.n_total;
#if !(RTX_PREP_ABLATE & 4)
  while (k < g.n_total && grid_x(g, k) <= v) ++k;
  while (k > 0 && grid_x(g, k - 1) > v) --k;
#endif
  return k;
}

__device__ __forceinline__ int clamp_local(long long ig, const GridDev& g) {
  long long l = ig - g.offset;
  if (l < 0) l = 0;
  if (l > g.n) l = g.n;
  return (int)l;
}

// Local centre index clamped to [-1e8, n+1e8]: with n <= 2e9 and zw <= 4e7 every i - i0, lo - i0 and
// i0 +- zw the line-sum forms stays inside int32. A centre that far outside reaches the shard only through a wide
// OmegaWing; its record's c is then taken at the clamped index (line_prep_kernel), so its far wing stays exact.
__device__ __forceinline__ int sat_local(long long v, long long n) {
  const long long M = 100000000LL;
  return (int)(v < -M ? -M : (v > n + M ? n + M : v));
}

// ---- per-line physics, shared by the grid prologue (line_prep_kernel) and the axis prologue (line_prep_axis_kernel) ----
struct LinePhys {
  double GammaD, Gamma0, Shift0, W;
  double Gam2;  // MIX only: the speed-dependent width of profile SDVOIGT (misc/hapi.py:10884-10890)
};

// Column set c of line l for the mixed prologue -- 0 air, 1 self, 2 + j extra set j -- with the reference's fallbacks
// (misc/hapi.py:11097-11125): an absent delta / deltap is 0, an absent n is n_air, and so is a self n of 0. The extra sets
// carry theirs already (rtx_lines_set_broadeners).
struct DilCols {
  double g, n, d, dp;
};
__device__ __forceinline__ DilCols dil_cols(const PrepArgs& a, int c, long long l) {
  DilCols r;
  if (c == 0) {
    r.g = a.gamma_air[l]; r.n = a.n_air[l]; r.d = a.delta_air[l]; r.dp = a.deltap_air ? a.deltap_air[l] : 0.0;
  } else if (c == 1) {
    double ns = a.n_self ? a.n_self[l] : a.n_air[l];
    if (a.n_self && ns == 0.0) ns = a.n_air[l];
    r.g = a.gamma_self[l]; r.n = ns;
    r.d = a.delta_self ? a.delta_self[l] : 0.0;
    r.dp = a.deltap_self ? a.deltap_self[l] : 0.0;
  } else {
    const size_t o = (size_t)(c - 2) * (size_t)a.n_lines + (size_t)l;
    r.g = a.x_gamma[o]; r.n = a.x_n[o]; r.d = a.x_delta[o]; r.dp = a.x_deltap[o];
  }
  return r;
}
__device__ __forceinline__ double dil_sd(const PrepArgs& a, int c, long long l) {
  if (c == 0) return a.sd_air ? a.sd_air[l] : 0.0;
  if (c == 1) return a.sd_self ? a.sd_self[l] : 0.0;
  return a.x_sd[(size_t)(c - 2) * (size_t)a.n_lines + (size_t)l];
}

// GammaD, Gamma0 / Shift0 over the diluent mix and the window half-width OmegaWingF of line l (species sp) in layer k at
// (T, p). MIX = false: the call-wide dil_air / dil_self; MIX = true: the per-(diluent, species, layer) fractions.
template <bool MIX>
__device__ __forceinline__ LinePhys line_phys(const PrepArgs& a, long long l, double T, double p, double mass, double nu, int sp,
                                              int k) {
  LinePhys r;
  // GammaD, misc/hapi.py:11085-11087
  const double m = mass * H_CMASSMOL * 1000.0;
  double GammaD = sqrt(2.0 * H_CBOLTS * T * log(2.0) / m / (H_CC * H_CC)) * nu;
  if (a.profile == RTX_PROFILE_DOPPLER)  // absorptionCoefficient_Doppler's own SI constants, misc/hapi.py:11534-11538
    GammaD = (1.1774100225 / 2.99792458e8) * sqrt(1.3806503e-23 / 1.66053873e-27) * sqrt(T) * nu / sqrt(mass);
  // Gamma0 / Shift0 over the diluent mix, misc/hapi.py:11090-11128
  double Gamma0 = 0.0, Shift0 = 0.0;
  const double tr = H_TREF / T;
  // (Tref/T)^n as exp(n log(Tref/T)): the logarithm is the same for every line of the layer; |n log(Tref/T)| < 1, so the
  // result is within 2 ulp of pow's (whose extended-precision logarithm is 200 fp64 instructions of this kernel's ~1000)
  const double ltr = log(tr);
  r.Gam2 = 0.0;
  if (MIX) {
    // misc/hapi.py:11090-11128 (Gamma2 :10884-10890, from each set's un-scaled gamma) in the caller's diluent order; a zero
    // fraction is skipped, as the air / self prologue skips a zero dil_air / dil_self
    for (int d = 0; d < a.n_dil; ++d) {
      const double f = a.frac[((size_t)d * a.n_species + sp) * a.n_layers + k];
      if (f == 0.0) continue;
      const int c = a.dil_idx[d];
      const DilCols q = dil_cols(a, c, l);
      Gamma0 += f * (q.g * p / 1.0 * exp(q.n * ltr));
      Shift0 += f * ((q.d + q.dp * (T - H_TREF)) * p / 1.0);
      if (a.profile == RTX_PROFILE_SDVOIGT) r.Gam2 += f * (dil_sd(a, c, l) * p) * q.g;
    }
  } else {
  if (a.dil_air != 0.0) {
#if RTX_PREP_ABLATE & 1  /* timing experiments only */
    Gamma0 += a.dil_air * (a.gamma_air[l] * p / 1.0 * (tr * a.n_air[l]));
#else
    Gamma0 += a.dil_air * (a.gamma_air[l] * p / 1.0 * exp(a.n_air[l] * ltr));
#endif
    const double dp = a.deltap_air ? a.deltap_air[l] : 0.0;
    Shift0 += a.dil_air * ((a.delta_air[l] + dp * (T - H_TREF)) * p / 1.0);
  }
  if (a.dil_self != 0.0) {
    double ns = a.n_self ? a.n_self[l] : a.n_air[l];
    if (a.n_self && ns == 0.0) ns = a.n_air[l];
    Gamma0 += a.dil_self * (a.gamma_self[l] * p / 1.0 * exp(ns * ltr));
    const double ds = a.delta_self ? a.delta_self[l] : 0.0;
    const double dps = a.deltap_self ? a.deltap_self[l] : 0.0;
    Shift0 += a.dil_self * ((ds + dps * (T - H_TREF)) * p / 1.0);
  }
  }  // !MIX
  if (a.profile == RTX_PROFILE_DOPPLER) {  // no pressure broadening; Shift0 = delta_air * p (misc/hapi.py:11543), set by the host through dil_air = 1 / 0 (LineShift)
    Gamma0 = 0.0;
    Shift0 = a.dil_air * a.delta_air[l] * p;
  }
  // OmegaWingF and the window: Voigt misc/hapi.py:11131-11134, Lorentz :11364, Doppler :11540
  r.W = a.profile == RTX_PROFILE_LORENTZ   ? fmax(a.omega_wing, a.omega_wing_hw * Gamma0)
        : a.profile == RTX_PROFILE_DOPPLER ? fmax(a.omega_wing, a.omega_wing_hw * GammaD)
                                           : fmax(a.omega_wing, fmax(a.omega_wing_hw * Gamma0, a.omega_wing_hw * GammaD));
  r.GammaD = GammaD; r.Gamma0 = Gamma0; r.Shift0 = Shift0;
  return r;
}

// S(T): EnvironmentDependency_Intensity, misc/hapi.py:10169-10175 (SigmaTref/SigmaT = qratio)
__device__ __forceinline__ double line_strength(const PrepArgs& a, long long l, double T, double nu, double qratio) {
  const double el = a.elower[l];
#if RTX_PREP_ABLATE & 2
  const double ch = (-H_C2 * el / T) * (1.0 - (-H_C2 * nu / T));
  const double zn = (-H_C2 * el / H_TREF) * (1.0 - (-H_C2 * nu / H_TREF));
#else
  const double ch = exp(-H_C2 * el / T) * (1.0 - exp(-H_C2 * nu / T));
  const double zn = a.zn[l];  // exp(-H_C2 * el / H_TREF) * (1.0 - exp(-H_C2 * nu / H_TREF)), from table creation (lines_zn_kernel)
#endif
  return a.sw[l] * qratio * ch / zn;
}

// profile parameters: pcqsdhc PART1, misc/hapi.py:9900-9915 -- every field of the two records that does not depend on the
// spectral axis (r.a, r.c, r.i0, r.lo, r.hi, r.zw are the caller's).
// Lorentz (PROFILE_LORENTZ, misc/hapi.py:10150): with x = (nu - sg0)/Gamma0 the profile is (1/(pi Gamma0)) / (x^2 + 1)
// = (x^2 K + K) / ((x^2 + 2) x^2 + 1), i.e. the line-sum's far-wing rational with b1 = 2, b0 = 1, Ay = Ay0 = K:
// the same kernels evaluate it everywhere (no band: y is set to 15), poles at |nu - sg0| = Gamma0 as for Voigt.
// Doppler (PROFILE_DOPPLER, :10160) is the Voigt profile at y = 0: Re w(x) = exp(-x^2); the band |x| < 15 goes
// through the fp64 Weideman pass, beyond it the reference's exp(-225) = 1e-98 is dropped.
__device__ __forceinline__ void line_profile(int profile, const LinePhys& ph, double w, double S, bool dropped, double scale,
                                             double sg0, LineRec& r, LineRec64& r64) {
  const bool lor = profile == RTX_PROFILE_LORENTZ;
  const double cte = lor ? 1.0 / ph.Gamma0 : sqrt(log(2.0)) / ph.GammaD;
  const double y = lor ? 15.0 : ph.Gamma0 * cte;
  const double A = dropped ? 0.0 : (lor ? w * S * cte / M_PI * scale : w * S * cte / sqrt(M_PI) * scale);
  const double yh = y * y + 0.5;
  r.b1 = lor ? 2.0f : (float)(2.0 * (y * y) - 1.0);
  r.b0 = lor ? 1.0f : (float)(yh * yh);
  r.Ay = lor ? (float)A : (float)(A * y * 0.56418958354775628);
  r.Ay0 = lor ? (float)A : (float)(A * y * 0.56418958354775628 * yh);
  r.y = (float)y;
  r.A = (float)A;
  r64.sg0 = sg0; r64.cte = cte; r64.y = y; r64.A = A;
}

// maximum of the 256 threads' v -> one atomicMax per block
__device__ __forceinline__ void block_max_hw(int v, int* dst) {
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_down(v, off));
  __shared__ int s_hw[4];
  if ((threadIdx.x & 63) == 0) s_hw[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int m = max(max(s_hw[0], s_hw[1]), max(s_hw[2], s_hw[3]));
    if (m > 0) atomicMax(dst, m);
  }
}

// WIN: every window (W, hence lo / hi, maxhw and the skip test) is that of the line at the layer's window temperature
// a.Twin[k] (rtx_line_prep_window); strengths, widths and shifts stay at T. WIN = false is the reference's prologue.
// MIX: Gamma0 / Shift0 / Gamma2 over the per-(diluent, species, layer) fractions (rtx_line_prep_mix); everything else as MIX = false.
template <bool ENV_ARGS, bool WIN, bool MIX>
__global__ __launch_bounds__(256) void line_prep_kernel(PrepArgs a) {
  const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int k = blockIdx.y;
  int my_hw = 0;
  // ENV_ARGS: a.T ... a.mass hold element offsets into a.env (kernel-argument segment), else device pointers
  const double* eT = ENV_ARGS ? a.env + (size_t)a.T : a.T;
  const double* ep = ENV_ARGS ? a.env + (size_t)a.p : a.p;
  const double* eq = ENV_ARGS ? a.env + (size_t)a.qratio : a.qratio;
  const double* ew = ENV_ARGS ? a.env + (size_t)a.weight : a.weight;
  const double* em = ENV_ARGS ? a.env + (size_t)a.mass : a.mass;
  if (l < a.n_lines) {
    const GridDev& g = a.g;
    const double T = eT[k], p = ep[k];
    const double nu = a.nu[l];
    const int sp = a.species[l];
    const double w = ew[(size_t)sp * a.n_layers + k];
    const LinePhys ph = line_phys<MIX>(a, l, T, p, em[sp], nu, sp, k);
    const double GammaD = ph.GammaD, Gamma0 = ph.Gamma0, Shift0 = ph.Shift0;
    const double W = WIN ? line_phys<MIX>(a, l, a.Twin[k], p, em[sp], nu, sp, k).W : ph.W;
    long long glo = grid_bisect_right(g, nu - W);
    long long ghi = grid_bisect_right(g, nu + W);
    int lo = clamp_local(glo, g), hi = clamp_local(ghi, g);
    const double sg0 = nu + Shift0;
    const long long M = 1000000000LL;
    if (k == 0) {
      long long gic = llrint((nu - g.xmin) / g.step);
      if (gic < -M) gic = -M;
      if (gic > M) gic = M;
      a.ic[l] = sat_local(gic - g.offset, g.n);
    }
    // A wavenumber SHARD (one rank of N) is reached by ~1/N of the table, but every rank runs this prologue over all of it
    // (the candidate ranges, hence the order of the fp32 sums, must not depend on where the shard is cut: maxhw below is a
    // maximum over the whole table). A line whose window ends a grid step or more outside the shard contributes nothing
    // here and its record is read at most as a rejected tile candidate, so the
    // rest of the work (S(T): four fp64 exponentials, the profile constants, 80 bytes of records) is skipped for it. Not
    // with an intensity threshold (whether the line counts for maxhw then depends on S) and not for the SD-Voigt records.
    const bool pre_dropped = !(w != 0.0) || !(GammaD > 0.0) || (a.profile == RTX_PROFILE_LORENTZ && !(Gamma0 > 0.0));
    const bool outside = nu + W < grid_x(g, g.offset) - g.step || nu - W > grid_x(g, g.offset + g.n - 1) + g.step;
    const bool skip = outside && !(a.thresh > 0.0) && a.profile != RTX_PROFILE_SDVOIGT;
    if (skip) {
      long long gi0 = llrint((sg0 - g.xmin) / g.step);
      if (gi0 < -M) gi0 = -M;
      if (gi0 > M) gi0 = M;
      const size_t o = (size_t)k * (size_t)a.n_lines + (size_t)l;
      // lo = hi = 0 rejects it; the other fields are finite and give a zero contribution with a non-zero denominator (the
      // line-sum fills the empty slots of a group of 8 from whatever candidate lane is at hand and zeroes the numerator)
      LineRec r;
      r.a = 0.f; r.c = 0.f; r.b1 = 0.f; r.b0 = 1.f; r.Ay = 0.f; r.Ay0 = 0.f; r.y = 15.f; r.A = 0.f;
      r.i0 = sat_local(gi0 - g.offset, g.n); r.lo = 0; r.hi = 0; r.zw = 0;
      a.rec[o] = r;
      a.win[o] = make_int2(0, 0);
      if (!pre_dropped && ghi > glo) {
        double hw = ceil(W / g.step) + 2.0;
        my_hw = hw > 1.0e9 ? 1000000000 : (int)hw;
      }
    } else {
    const double S = line_strength(a, l, T, nu, eq[(size_t)sp * a.n_layers + k]);
    const bool dropped = pre_dropped || (S < a.thresh);
    if (dropped || hi <= lo) { lo = 0; hi = 0; }
    LineRec r;
    LineRec64 r64;
    line_profile(a.profile, ph, w, S, dropped, a.scale, sg0, r, r64);
    const double cte = r64.cte, y = r64.y;
    // nearest grid index to the shifted centre (global), then the residual in fp64
    long long gi0 = llrint((sg0 - g.xmin) / g.step);
    if (gi0 < -M) gi0 = -M;
    if (gi0 > M) gi0 = M;
    r.i0 = sat_local(gi0 - g.offset, g.n);
    // x at the record's centre index: gi0 (|.| <= a/2 when inside the grid) unless the local clamp moved it -- a centre
    // over 1e8 points outside the shard whose window still reaches in (OmegaWing) -- so that x = u a + c is the line's own
    const double frac_x = (grid_x(g, g.offset + (long long)r.i0) - sg0) * cte;
    const double ax = g.step * cte;
    r.a = (float)ax;
    r.c = (float)frac_x;
    r.lo = lo;
    r.hi = hi;
    // half-width (grid points) of the band that can satisfy |x|+y<15 (hum1_wei switch, misc/hapi.py:9840)
    int zw = 0;
    if (y < 15.0 && hi > lo) {
      double z = ceil((15.0 - y) / ax) + 2.0;
      zw = z > 4.0e7 ? 40000000 : (int)z;
    }
    r.zw = zw;
    if (zw > 0 && r.y < 1.0f) a.smally[k] = 1;  // benign race: every writer stores 1
    const size_t o = (size_t)k * (size_t)a.n_lines + (size_t)l;
#if !(RTX_PREP_ABLATE & 8)
    a.rec[o] = r;
#ifndef RTX_PREP_ABLATE_REC64
    a.rec64[o] = r64;
#endif
#endif
    a.win[o] = make_int2(lo, hi);
    if (a.profile == RTX_PROFILE_SDVOIGT) {
      // Gamma2 = sum_species abun * SD_species * p/pref * gamma_species(Tref) (misc/hapi.py:10884-10890); Shift2 = 0
      double Gam2 = 0.0;
      if (MIX) {
        Gam2 = ph.Gam2;
      } else {
        if (a.dil_air != 0.0 && a.sd_air) Gam2 += a.dil_air * (a.sd_air[l] * p) * a.gamma_air[l];
        if (a.dil_self != 0.0 && a.sd_self) Gam2 += a.dil_self * (a.sd_self[l] * p) * a.gamma_self[l];
      }
      LineRecSD q;
      q.nu = nu; q.cte = cte; q.Gam0 = Gamma0; q.Shift0 = Shift0; q.Gam2 = Gam2; q.WS = dropped ? 0.0 : w * S;
      q.inv_Gam2 = Gam2 != 0.0 ? 1.0 / Gam2 : 0.0;
      q.csqrtY = Gam2 != 0.0 ? 1.0 / (2.0 * cte * Gam2) : 0.0;
      a.recsd[o] = q;
    }
    if (!dropped && ghi > glo) {
      // window half-width in grid points, measured from the unshifted centre, with margin. Taken over every live line
      // whose window meets the FULL axis, not only this shard: the per-tile candidate ranges -- hence the order of the
      // fp32 sums -- then do not depend on where a shard is cut (tile-aligned shards reproduce the full grid's bits)
      double hw = ceil(W / g.step) + 2.0;
      my_hw = hw > 1.0e9 ? 1000000000 : (int)hw;
    }
    }  // !skip
  }
  block_max_hw(my_hw, &a.maxhw[k]);
}

// ---- the prologue on an explicit axis (rtx_line_prep_axis) --------------------------------------------------------------
// bisect.bisect_right (RIGHT) / bisect_left of v on the device copy of the axis, with Python's comparisons: the number of
// points <= v / < v.
template <bool RIGHT>
__device__ long long axis_bisect(const double* __restrict__ X, long long nx, double v) {
  long long lo = 0, hi = nx;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (RIGHT ? v < X[mid] : !(X[mid] < v)) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// One thread per (line, layer), as line_prep_kernel, with the same physics (line_phys, line_strength, line_profile). The
// window is bisect_right(X, nu -+ W) on the axis itself, so every line's support is the reference's point for point
// (misc/hapi.py:11133-11134). The candidate ranges of tile_ranges_kernel come from index-space inputs: ic[l] =
// bisect_right(X, nu_l) (non-decreasing: the table is sorted by nu) and maxhw[k] = max over live lines of
// max(ic - lo, hi - ic) + 1 points, so the bracket [ia - maxhw, ib - 1 + maxhw] of centre indices still holds every line
// whose window meets tile [ia, ib). Records: LineRec's axis meanings (rtx_common.h); [i0, zw) = the indices within
// (15 - y + 0.01)/cte of the shifted centre -- the points that can satisfy hum1_wei's |x|+y<15 (misc/hapi.py:9840), with a
// margin of 0.01 in x far above the fp32 error of the line-sum's x.
template <bool ENV_ARGS, bool MIX>
__global__ __launch_bounds__(256) void line_prep_axis_kernel(PrepArgs a) {
  const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int k = blockIdx.y;
  int my_hw = 0;
  const double* eT = ENV_ARGS ? a.env + (size_t)a.T : a.T;
  const double* ep = ENV_ARGS ? a.env + (size_t)a.p : a.p;
  const double* eq = ENV_ARGS ? a.env + (size_t)a.qratio : a.qratio;
  const double* ew = ENV_ARGS ? a.env + (size_t)a.weight : a.weight;
  const double* em = ENV_ARGS ? a.env + (size_t)a.mass : a.mass;
  if (l < a.n_lines) {
    const double T = eT[k], p = ep[k];
    const double nu = a.nu[l];
    const int sp = a.species[l];
    const double w = ew[(size_t)sp * a.n_layers + k];
    const LinePhys ph = line_phys<MIX>(a, l, T, p, em[sp], nu, sp, k);
    const double S = line_strength(a, l, T, nu, eq[(size_t)sp * a.n_layers + k]);
    const bool dropped = !(w != 0.0) || !(ph.GammaD > 0.0) || (a.profile == RTX_PROFILE_LORENTZ && !(ph.Gamma0 > 0.0)) ||
                         (S < a.thresh);
    long long lo = axis_bisect<true>(a.X, a.nx, nu - ph.W), hi = axis_bisect<true>(a.X, a.nx, nu + ph.W);
    if (dropped || hi <= lo) { lo = 0; hi = 0; }
    const long long ic = axis_bisect<true>(a.X, a.nx, nu);
    if (k == 0) a.ic[l] = (int)ic;
    const double sg0 = nu + ph.Shift0;
    LineRec r;
    LineRec64 r64;
    line_profile(a.profile, ph, w, S, dropped, a.scale, sg0, r, r64);
    r.a = (float)r64.cte;
    r.c = 0.f;
    long long zlo = 0, zhi = 0;
    if (r64.y < 15.0 && hi > lo) {
      const double wz = (15.0 - r64.y + 0.01) / r64.cte;
      zlo = axis_bisect<false>(a.X, a.nx, sg0 - wz);
      zhi = axis_bisect<true>(a.X, a.nx, sg0 + wz);
      zlo = zlo < lo ? lo : zlo;
      zhi = zhi > hi ? hi : zhi;
      if (zhi < zlo) zhi = zlo;
    }
    r.i0 = (int)zlo; r.zw = (int)zhi;
    r.lo = (int)lo; r.hi = (int)hi;
    const size_t o = (size_t)k * (size_t)a.n_lines + (size_t)l;
    a.rec[o] = r;
    a.rec64[o] = r64;
    a.win[o] = make_int2((int)lo, (int)hi);
    if (hi > lo) my_hw = (int)(ic - lo > hi - ic ? ic - lo : hi - ic) + 1;
  }
  block_max_hw(my_hw, &a.maxhw[k]);
}

// ---- hot tiles: host-side bound on the extra parts (rtx_common.h) ------------------------------------------------------
// No window of any line in any layer is wider than W = max(OmegaWing, HW * Gamma0_max, HW * GammaD_max) (misc/hapi.py:11131
// with the column extremes of the table and the layer extremes of this call), and windows are centred on the UNSHIFTED
// centres, so a tile [x_a, x_b] has at most count(nu in [x_a - W, x_b + W]) candidates: one sweep over the sorted host
// copy of the centres. The work list and the partial-tile workspace are sized from that bound -- they cannot overflow, and
// nothing is read back from the device. The sweep (~0.1 ms for 100 000 lines) is redone only when the grid changes or a call
// needs a wider window than the cached bound was made for (25 % headroom). A table that cannot have a hot tile (every
// uniform table of the benchmarks) has bound 0 and never launches the two extra kernels.
// Bound on Gamma0 over every line and layer of a call with the call-wide fractions dil_air / dil_self.
static double gamma0_bound(const rtx_lines* L, int n_layers, const double* T_h, const double* p_h, double dil_air, double dil_self) {
  double g0 = 0.0;
  for (int k = 0; k < n_layers; ++k) {
    const double tr = H_TREF / T_h[k];
    g0 = fmax(g0, p_h[k] * fmax(pow(tr, L->n_lo), pow(tr, L->n_hi)));
  }
  return g0 * (fabs(dil_air) * L->ga_max + fabs(dil_self) * L->gs_max);
}

// The same with per-(diluent, species, layer) fractions: max over species and layers of p sum_d |f_d| gmax_d (Tref/T)^n_d, with
// the |gamma| maximum and the n range of every column set used.
static double gamma0_bound_mix(const rtx_lines* L, int n_layers, const double* T_h, const double* p_h, int n_dil, const int32_t* dil_h,
                               const double* frac_h) {
  double g0 = 0.0;
  const int ns = L->n_species;
  for (int k = 0; k < n_layers; ++k) {
    const double tr = H_TREF / T_h[k];
    for (int s = 0; s < ns; ++s) {
      double sum = 0.0;
      for (int d = 0; d < n_dil; ++d) {
        const int c = dil_h[d];
        const double gm = c == 0 ? L->ga_max : c == 1 ? L->gs_max : L->x_gmax[c - 2];
        const double lo = c == 0 ? L->na_lo : c == 1 ? L->ns_lo : L->x_nlo[c - 2];
        const double hi = c == 0 ? L->na_hi : c == 1 ? L->ns_hi : L->x_nhi[c - 2];
        sum += fabs(frac_h[((size_t)d * ns + s) * n_layers + k]) * gm * fmax(pow(tr, lo), pow(tr, hi));
      }
      g0 = fmax(g0, p_h[k] * sum);
    }
  }
  return g0;
}

// g0: bound on Gamma0 over the call (gamma0_bound / gamma0_bound_mix)
static int rtx_split_bound(rtx_prep* P, const rtx_lines* L, const rtx_grid* g, int n_layers, const double* T_h, const double* mass_h,
                           double g0, double omega_wing, double omega_wing_hw, int profile) {
  if (L->n == 0 || g->n == 0) { P->split_bound = 0; return 0; }
  double t_max = 0.0;
  for (int k = 0; k < n_layers; ++k) t_max = fmax(t_max, T_h[k]);
  double m_min = 1e300;
  for (int s = 0; s < L->n_species; ++s)
    if (mass_h[s] > 0.0) m_min = fmin(m_min, mass_h[s]);
  if (!(m_min < 1e300)) m_min = 1.0;
  const double nu_max = L->nu_host.back();
  double gd = sqrt(2.0 * H_CBOLTS * t_max * log(2.0) / (m_min * H_CMASSMOL * 1000.0) / (H_CC * H_CC)) * fabs(nu_max);
  if (profile == RTX_PROFILE_DOPPLER) gd = (1.1774100225 / 2.99792458e8) * sqrt(1.3806503e-23 / 1.66053873e-27) * sqrt(t_max) * fabs(nu_max) / sqrt(m_min);
  const double W = fmax(omega_wing, fmax(omega_wing_hw * g0, omega_wing_hw * gd)) + 2.0 * g->step;
  const bool same_grid = P->split_xmin == g->xmin && P->split_step == g->step && P->split_off == g->offset && P->split_n == g->n;
  if (same_grid && P->split_lines == (const void*)L && P->split_W > 0.0 && W <= P->split_W && n_layers <= P->split_layers) return 0;  // the cached bound covers this call
  const double Wc = 1.25 * W;
  const int tile = rtx_voigt_tile_points();
  const long long n_tiles = (g->n + tile - 1) / tile;
  long long extra = 0, a = 0, b = 0;
  for (long long t = 0; t < n_tiles; ++t) {
    const double xa = g->xmin + (double)(g->offset + t * tile) * g->step - Wc;
    long long i_end = g->offset + (t + 1) * tile;
    if (i_end > g->offset + g->n) i_end = g->offset + g->n;
    const double xb = g->xmin + (double)i_end * g->step + Wc;
    while (a < L->n && L->nu_host[a] < xa) ++a;
    if (b < a) b = a;
    while (b < L->n && L->nu_host[b] <= xb) ++b;
    const long long cnt = b - a;
    if (cnt > RTX_SPLIT_MIN) extra += (cnt - 1) / RTX_SPLIT_PART;
  }
  extra *= n_layers;
  if (extra > 1000000LL)  // 4 GB of partial tiles: callers with many states per launch split the launch (afit_xs.py)
    RTX_FAIL("hot-tile work list of %lld items (over 1000000): fewer layers / states per call, or a shorter grid shard", extra);
  // rare growth (a new table / grid / much wider wings); the two go together: the list's capacity stands for both
  if (P->items.reserve((size_t)extra) || P->part_ws.reserve((size_t)extra * (size_t)tile)) {
    P->items.reset(); P->part_ws.reset();
    P->split_bound = 0; P->split_W = 0.0;
    return 1;
  }
  P->split_bound = extra;
  P->split_W = Wc; P->split_xmin = g->xmin; P->split_step = g->step; P->split_off = g->offset; P->split_n = g->n;
  P->split_layers = n_layers;
  P->split_lines = (const void*)L;
  return 0;
}

extern "C" int64_t rtx_prep_split_bound(const rtx_prep* P) { return P ? P->split_bound : -1; }

// Checks and per-layer tables common to both prologues: validates the call, packs T | p | qratio | weight | mass into the
// kernel arguments (or copies them into the prep object when they do not fit), clears maxhw / smally / n_items and fills
// every field of `a` that does not depend on the spectral axis.
static int prep_begin(rtx_prep* P, const rtx_lines* L, int n_layers, const double* T_h, const double* p_atm_h,
                      const double* qratio_h, const double* weight_h, const double* mass_h, double dil_air, double dil_self,
                      double omega_wing, double omega_wing_hw, double intensity_threshold, double scale, int profile,
                      hipStream_t st, PrepArgs& a, bool& env_args) {
  if (P->n_lines != L->n) RTX_FAIL("prep object was created for %lld lines, table has %lld", P->n_lines, L->n);
  if (n_layers < 1 || n_layers > P->max_layers) RTX_FAIL("n_layers=%d outside [1,%d]", n_layers, P->max_layers);
  if (!T_h || !p_atm_h || !qratio_h || !weight_h || !mass_h) RTX_FAIL("a per-layer input is NULL");
  if (!(scale > 0.0)) RTX_FAIL("scale must be > 0");
  for (int k = 0; k < n_layers; ++k)
    if (!(T_h[k] > 0.0) || !(p_atm_h[k] >= 0.0)) RTX_FAIL("layer %d: T=%g p=%g not physical", k, T_h[k], p_atm_h[k]);
  const int ns = L->n_species;
  const size_t nT = (size_t)n_layers, nQ = (size_t)ns * n_layers;
  if (2 * nT + 2 * nQ + ns > P->env.cap()) RTX_FAIL("environment tables exceed prep capacity");
  env_args = 2 * nT + 2 * nQ + ns <= RTX_ENV_MAX;
  double* d = P->env.get();
  if (!env_args) {
    // pageable-source async copies are staged by the runtime before returning: caller may reuse its arrays
    RTX_HIP(hipMemcpyAsync(d, T_h, nT * sizeof(double), hipMemcpyHostToDevice, st));
    RTX_HIP(hipMemcpyAsync(d + nT, p_atm_h, nT * sizeof(double), hipMemcpyHostToDevice, st));
    RTX_HIP(hipMemcpyAsync(d + 2 * nT, qratio_h, nQ * sizeof(double), hipMemcpyHostToDevice, st));
    RTX_HIP(hipMemcpyAsync(d + 2 * nT + nQ, weight_h, nQ * sizeof(double), hipMemcpyHostToDevice, st));
    RTX_HIP(hipMemcpyAsync(d + 2 * nT + 2 * nQ, mass_h, ns * sizeof(double), hipMemcpyHostToDevice, st));
  }
  RTX_HIP(hipMemsetAsync(P->maxhw.get(), 0, P->maxhw.cap() * sizeof(int), st));  // maxhw, smally and n_items
  a.nu = L->nu.get(); a.sw = L->sw.get(); a.elower = L->elower.get(); a.gamma_air = L->gamma_air.get(); a.gamma_self = L->gamma_self.get();
  a.n_air = L->n_air.get(); a.n_self = L->n_self.get(); a.delta_air = L->delta_air.get(); a.deltap_air = L->deltap_air.get();
  a.delta_self = L->delta_self.get(); a.species = L->species.get();
  a.sd_air = L->sd_air.get(); a.sd_self = L->sd_self.get(); a.deltap_self = L->deltap_self.get(); a.recsd = P->recsd.get(); a.zn = L->zn.get();
  a.n_lines = L->n; a.n_layers = n_layers; a.n_species = ns;
  if (env_args) {  // offsets (in doubles) into a.env, carried in the pointer fields
    a.T = (const double*)(size_t)0; a.p = (const double*)nT; a.qratio = (const double*)(2 * nT);
    a.weight = (const double*)(2 * nT + nQ); a.mass = (const double*)(2 * nT + 2 * nQ);
    memcpy(a.env, T_h, nT * sizeof(double));
    memcpy(a.env + nT, p_atm_h, nT * sizeof(double));
    memcpy(a.env + 2 * nT, qratio_h, nQ * sizeof(double));
    memcpy(a.env + 2 * nT + nQ, weight_h, nQ * sizeof(double));
    memcpy(a.env + 2 * nT + 2 * nQ, mass_h, ns * sizeof(double));
  } else {
    a.T = d; a.p = d + nT; a.qratio = d + 2 * nT; a.weight = d + 2 * nT + nQ; a.mass = d + 2 * nT + 2 * nQ;
  }
  a.dil_air = dil_air; a.dil_self = dil_self; a.omega_wing = omega_wing; a.omega_wing_hw = omega_wing_hw;
  a.thresh = intensity_threshold; a.scale = scale; a.profile = profile;
  a.X = nullptr; a.nx = 0; a.Twin = nullptr;
  a.n_dil = 0; a.frac = nullptr;
  for (int d = 0; d < RTX_MIX_MAX; ++d) a.dil_idx[d] = 0;
  a.x_gamma = L->x_gamma.get(); a.x_n = L->x_n.get(); a.x_delta = L->x_delta.get(); a.x_deltap = L->x_deltap.get(); a.x_sd = L->x_sd.get();
  a.rec = P->rec.get(); a.rec64 = P->rec64.get(); a.ic = P->ic.get(); a.win = P->win.get(); a.maxhw = P->maxhw.get(); a.smally = P->smally;
  return 0;
}

// The diluent mix of rtx_line_prep_mix / _axis_mix: checks it and copies the fractions into the prep object's buffer. After prep_begin.
static int mix_begin(rtx_prep* P, const rtx_lines* L, int n_layers, int n_dil, const int32_t* dil_h, const double* frac_h,
                     hipStream_t st, PrepArgs& a) {
  if (n_dil < 0 || n_dil > RTX_MIX_MAX) RTX_FAIL("n_dil=%d outside [0,%d]", n_dil, RTX_MIX_MAX);
  if (n_dil > 0 && (!dil_h || !frac_h)) RTX_FAIL("diluent indices / fractions are NULL");
  for (int d = 0; d < n_dil; ++d)
    if (dil_h[d] < 0 || dil_h[d] >= 2 + L->n_extra)
      RTX_FAIL("diluent %d: column set %d outside [0,%d) (0 air, 1 self, 2.. rtx_lines_set_broadeners)", d, dil_h[d], 2 + L->n_extra);
  const size_t nf = (size_t)n_dil * (size_t)L->n_species * (size_t)n_layers;
  if (nf) {  // sized once, for the most a call may bring
    if (P->frac.reserve((size_t)RTX_MIX_MAX * (size_t)L->n_species * (size_t)P->max_layers)) return 1;
    RTX_HIP(hipMemcpyAsync(P->frac.get(), frac_h, nf * sizeof(double), hipMemcpyHostToDevice, st));  // staged before returning
  }
  a.n_dil = n_dil;
  for (int d = 0; d < n_dil; ++d) a.dil_idx[d] = dil_h[d];
  a.frac = P->frac.get();
  return 0;
}

// ---- host drivers of the prologue ------------------------------------------------------------------------------------
// The diluents of rtx_line_prep_mix / _axis_mix (NULL: the call-wide dil_air / dil_self).
struct MixIn {
  int n_dil;
  const int32_t* dil;
  const double* frac;
};
// What every prologue takes besides its spectral axis.
struct PrepIn {
  int n_layers;
  const double *T_h, *p_atm_h, *qratio_h, *weight_h, *mass_h;
  double dil_air, dil_self;
  const MixIn* mix;
  double omega_wing, omega_wing_hw, intensity_threshold, scale;
  int profile;
  hipStream_t st;
};

// First half of a prologue: the checks and per-layer tables (prep_begin), then the diluent mix.
static int prep_start(rtx_prep* P, const rtx_lines* L, const PrepIn& in, PrepArgs& a, bool& env_args) {
  if (prep_begin(P, L, in.n_layers, in.T_h, in.p_atm_h, in.qratio_h, in.weight_h, in.mass_h, in.dil_air, in.dil_self, in.omega_wing,
                 in.omega_wing_hw, in.intensity_threshold, in.scale, in.profile, in.st, a, env_args))
    return 1;
  return in.mix ? mix_begin(P, L, in.n_layers, in.mix->n_dil, in.mix->dil, in.mix->frac, in.st, a) : 0;
}

// Second half: notes what ran on the prep object and launches the kernel, one thread per (line, layer). The kernel is
// line_prep_axis_kernel<env_args, mix> on an axis, else line_prep_kernel<env_args, a.Twin given, mix> (a.Twin excludes mix).
static int prep_launch(rtx_prep* P, const rtx_lines* L, const PrepIn& in, bool axis, bool empty, bool env_args, const PrepArgs& a) {
  typedef void (*Kernel)(PrepArgs);
  static const Kernel grid_k[2][3] = {
      {line_prep_kernel<false, false, false>, line_prep_kernel<false, false, true>, line_prep_kernel<false, true, false>},
      {line_prep_kernel<true, false, false>, line_prep_kernel<true, false, true>, line_prep_kernel<true, true, false>}};
  static const Kernel axis_k[2][2] = {{line_prep_axis_kernel<false, false>, line_prep_axis_kernel<false, true>},
                                      {line_prep_axis_kernel<true, false>, line_prep_axis_kernel<true, true>}};
  P->n_layers = in.n_layers;
  P->scale = in.scale;
  P->axis = axis;
  P->dT = 0;  // rtx_line_prep_dt sets it once its derivative records are enqueued too
  if (empty) return 0;
  const Kernel k = axis ? axis_k[env_args][in.mix != nullptr] : grid_k[env_args][a.Twin ? 2 : in.mix ? 1 : 0];
  hipLaunchKernelGGL(k, dim3((unsigned)((L->n + 255) / 256), (unsigned)in.n_layers), dim3(256), 0, in.st, a);
  RTX_LAUNCH_CHECK();
  return 0;
}

// Grid prologue of rtx_line_prep_profile, rtx_line_prep_mix (in.mix) and rtx_line_prep_window (T_win_h: every window, hence
// the candidate half-widths and the hot-tile bound, at those temperatures; its device copy belongs to the prep object).
// keep / keep_env: where the caller (rtx_line_prep_dt) receives the kernel arguments and how the per-layer tables travel.
static int line_prep_grid(rtx_prep* P, const rtx_lines* L, const rtx_grid* grid, const double* T_win_h, const PrepIn& in,
                          PrepArgs* keep = nullptr, bool* keep_env = nullptr) {
  if (!P || !L) RTX_FAIL("prep/lines is NULL");
  if (in.profile < RTX_PROFILE_VOIGT || in.profile > RTX_PROFILE_SDVOIGT) RTX_FAIL("profile=%d", in.profile);
  if (in.mix && in.profile == RTX_PROFILE_DOPPLER) RTX_FAIL("rtx_line_prep_mix: the Doppler profile takes no diluent");
  if (in.mix && T_win_h) RTX_FAIL("window temperatures and a diluent mix do not go together");
  if (in.profile == RTX_PROFILE_SDVOIGT && P->recsd.reserve((size_t)(P->n_lines > 0 ? P->n_lines : 1) * (size_t)P->max_layers)) return 1;
  if (rtx_check_grid(grid)) return 1;
  PrepArgs a;
  bool env_args = false;
  if (prep_start(P, L, in, a, env_args)) return 1;
  if (T_win_h) {
    if (P->twin.reserve((size_t)P->max_layers)) return 1;
    RTX_HIP(hipMemcpyAsync(P->twin.get(), T_win_h, (size_t)in.n_layers * sizeof(double), hipMemcpyHostToDevice, in.st));  // staged before returning
    a.Twin = P->twin.get();
  }
  const double* T_w = T_win_h ? T_win_h : in.T_h;
  const double g0 = in.mix ? gamma0_bound_mix(L, in.n_layers, T_w, in.p_atm_h, in.mix->n_dil, in.mix->dil, in.mix->frac)
                           : gamma0_bound(L, in.n_layers, T_w, in.p_atm_h, in.dil_air, in.dil_self);
  if (rtx_split_bound(P, L, grid, in.n_layers, T_w, in.mass_h, g0, in.omega_wing, in.omega_wing_hw, in.profile)) return 1;
  a.g = to_dev(grid);
  if (keep) { *keep = a; *keep_env = env_args; }
  return prep_launch(P, L, in, false, L->n == 0, env_args, a);
}

static int line_prep_axis(rtx_prep* P, const rtx_lines* L, const double* X_h, int64_t nx, const PrepIn& in) {
  if (!P || !L) RTX_FAIL("prep/lines is NULL");
  if (in.profile < RTX_PROFILE_VOIGT || in.profile > RTX_PROFILE_DOPPLER)
    RTX_FAIL("rtx_line_prep_axis: profile=%d (Voigt, Lorentz or Doppler; the speed-dependent sum needs a uniform grid)", in.profile);
  if (in.mix && in.profile == RTX_PROFILE_DOPPLER) RTX_FAIL("rtx_line_prep_axis_mix: the Doppler profile takes no diluent");
  const long long cap = P->max_tiles * (long long)rtx_voigt_tile_points();
  if (nx < 0 || nx > cap) RTX_FAIL("axis of %lld points outside the prep capacity [0, %lld]", (long long)nx, cap);
  if (nx > 0 && !X_h) RTX_FAIL("axis is NULL");
  for (int64_t i = 0; i < nx; ++i) {
    if (!isfinite(X_h[i])) RTX_FAIL("axis point %lld is not finite", (long long)i);
    if (i > 0 && X_h[i] < X_h[i - 1]) RTX_FAIL("axis must be non-decreasing (point %lld)", (long long)i);
  }
  PrepArgs a;
  bool env_args = false;
  if (prep_start(P, L, in, a, env_args)) return 1;
  if (P->X.reserve((size_t)nx)) return 1;
  if (nx > 0) RTX_HIP(hipMemcpyAsync(P->X.get(), X_h, (size_t)nx * sizeof(double), hipMemcpyHostToDevice, in.st));  // staged before returning
  P->nx = nx;
  a.X = P->X.get(); a.nx = nx;
  return prep_launch(P, L, in, true, L->n == 0 || nx == 0, env_args, a);
}

// The entry points: each packs its arguments and names its driver.
#define RTX_PREP_IN(dil_air, dil_self, mix, profile)                                                                          \
  PrepIn { n_layers, T_h, p_atm_h, qratio_h, weight_h, mass_h, dil_air, dil_self, mix, omega_wing, omega_wing_hw, intensity_threshold, \
           scale, profile, (hipStream_t)stream }

extern "C" int rtx_line_prep_profile(rtx_prep* P, const rtx_lines* L, const rtx_grid* grid, int n_layers, const double* T_h,
                             const double* p_atm_h, const double* qratio_h, const double* weight_h, const double* mass_h,
                             double dil_air, double dil_self, double omega_wing, double omega_wing_hw,
                             double intensity_threshold, double scale, int profile, void* stream) {
  return line_prep_grid(P, L, grid, nullptr, RTX_PREP_IN(dil_air, dil_self, nullptr, profile));
}

extern "C" int rtx_line_prep(rtx_prep* P, const rtx_lines* L, const rtx_grid* grid, int n_layers, const double* T_h,
                             const double* p_atm_h, const double* qratio_h, const double* weight_h, const double* mass_h,
                             double dil_air, double dil_self, double omega_wing, double omega_wing_hw,
                             double intensity_threshold, double scale, void* stream) {
  return line_prep_grid(P, L, grid, nullptr, RTX_PREP_IN(dil_air, dil_self, nullptr, RTX_PROFILE_VOIGT));
}

extern "C" int rtx_line_prep_mix(rtx_prep* P, const rtx_lines* L, const rtx_grid* grid, int n_layers, const double* T_h,
                                 const double* p_atm_h, const double* qratio_h, const double* weight_h, const double* mass_h,
                                 int n_dil, const int32_t* dil_h, const double* frac_h, double omega_wing, double omega_wing_hw,
                                 double intensity_threshold, double scale, int profile, void* stream) {
  const MixIn mix = {n_dil, dil_h, frac_h};
  return line_prep_grid(P, L, grid, nullptr, RTX_PREP_IN(0.0, 0.0, &mix, profile));
}

extern "C" int rtx_line_prep_axis(rtx_prep* P, const rtx_lines* L, const double* X_h, int64_t nx, int n_layers, const double* T_h,
                                  const double* p_atm_h, const double* qratio_h, const double* weight_h, const double* mass_h,
                                  double dil_air, double dil_self, double omega_wing, double omega_wing_hw,
                                  double intensity_threshold, double scale, int profile, void* stream) {
  return line_prep_axis(P, L, X_h, nx, RTX_PREP_IN(dil_air, dil_self, nullptr, profile));
}

extern "C" int rtx_line_prep_axis_mix(rtx_prep* P, const rtx_lines* L, const double* X_h, int64_t nx, int n_layers, const double* T_h,
                                      const double* p_atm_h, const double* qratio_h, const double* weight_h, const double* mass_h,
                                      int n_dil, const int32_t* dil_h, const double* frac_h, double omega_wing, double omega_wing_hw,
                                      double intensity_threshold, double scale, int profile, void* stream) {
  const MixIn mix = {n_dil, dil_h, frac_h};
  return line_prep_axis(P, L, X_h, nx, RTX_PREP_IN(0.0, 0.0, &mix, profile));
}

// The grid prologue with the windows held at other temperatures: the derivative of the truncated line-sum with every
// line's support fixed (rtx_tud_jacobian's dOD/dT). Everything but the windows is taken at T_h. With
// T_win_h == T_h the records are those of rtx_line_prep_profile.
extern "C" int rtx_line_prep_window(rtx_prep* P, const rtx_lines* L, const rtx_grid* grid, int n_layers, const double* T_h,
                                    const double* T_win_h, const double* p_atm_h, const double* qratio_h, const double* weight_h,
                                    const double* mass_h, double dil_air, double dil_self, double omega_wing, double omega_wing_hw,
                                    double intensity_threshold, double scale, int profile, void* stream) {
  if (!P || !L) RTX_FAIL("prep/lines is NULL");
  if (profile < RTX_PROFILE_VOIGT || profile > RTX_PROFILE_DOPPLER)
    RTX_FAIL("rtx_line_prep_window: profile=%d (Voigt, Lorentz or Doppler)", profile);
  if (rtx_check_grid(grid)) return 1;
  if (!T_win_h) RTX_FAIL("T_win_h is NULL");
  for (int k = 0; k < n_layers; ++k)
    if (!(T_win_h[k] > 0.0)) RTX_FAIL("layer %d: window temperature %g not physical", k, T_win_h[k]);
  return line_prep_grid(P, L, grid, T_win_h, RTX_PREP_IN(dil_air, dil_self, nullptr, profile));
}

// ---- rtx_line_prep_dt: the grid prologue plus the temperature-derivative records ---------------------------
// The base records, windows and candidate inputs are written by line_prep_kernel itself, launched exactly as
// rtx_line_prep_profile launches it: the same kernel on the same arguments, hence the same bits. A second kernel, one thread
// per (line, layer) again, then reads the line's fp64 record (cte, y, A) and forms the derivative records in fp64:
//   alpha = dln(qratio w)/dT + c2 E"/T^2 - (u/T)/(e^u - 1) - 1/(2T),  u = c2 nu/T  (S(T) of line_strength, cte ~ T^-1/2),
//   Gamma0' = -sum_d f_d gamma_d p (Tref/T)^n_d n_d / T,  Shift0' = sum_d f_d deltap_d p  (line_phys, d = air, self).
// A line without a window in the shard (dropped, empty, or skipped by the prologue) is never visited by the sum: zeros.
struct PrepDTArgs {
  const double* dlnsw;  // [n_species][n_layers], device copy
  LineRecDT* drec;
  LineRecDT64* drec64;
};
static_assert(sizeof(PrepArgs) + sizeof(PrepDTArgs) <= 4096, "the derivative prologue's kernel arguments must stay within 4 KB");

template <bool ENV_ARGS>
__global__ __launch_bounds__(256) void line_prep_dT_kernel(PrepArgs a, PrepDTArgs d) {
  const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int k = blockIdx.y;
  if (l >= a.n_lines) return;
  const double* eT = ENV_ARGS ? a.env + (size_t)a.T : a.T;
  const double* ep = ENV_ARGS ? a.env + (size_t)a.p : a.p;
  const size_t o = (size_t)k * (size_t)a.n_lines + (size_t)l;
  const int2 w = a.win[o];
  LineRecDT r;
  LineRecDT64 r64;
  r.alpha = r.sx = r.yp = r.h = r.Ap = r.y2 = 0.f; r.yh = 0.5f; r.y = 15.f;
  r64.alpha = r64.sx = r64.gy = r64.h = 0.0;
  if (w.y > w.x) {
    const LineRec64 Q = a.rec64[o];
    const double T = eT[k], p = ep[k];
    const double nu = a.nu[l];
    const int sp = a.species[l];
    const double ltr = log(H_TREF / T);
    double G0p = 0.0, Sp = 0.0;
    if (a.dil_air != 0.0) {
      const double na = a.n_air[l];
      G0p += a.dil_air * (a.gamma_air[l] * p * exp(na * ltr)) * na;
      Sp += a.dil_air * ((a.deltap_air ? a.deltap_air[l] : 0.0) * p);
    }
    if (a.dil_self != 0.0) {
      double ns = a.n_self ? a.n_self[l] : a.n_air[l];
      if (a.n_self && ns == 0.0) ns = a.n_air[l];
      G0p += a.dil_self * (a.gamma_self[l] * p * exp(ns * ltr)) * ns;
      Sp += a.dil_self * ((a.deltap_self ? a.deltap_self[l] : 0.0) * p);
    }
    G0p = -G0p / T;
    const double u = H_C2 * nu / T;
    const double h = 0.5 / T;
    r64.alpha = d.dlnsw[(size_t)sp * a.n_layers + k] + H_C2 * a.elower[l] / (T * T) - (u / T) / expm1(u) - h;
    r64.sx = Sp * Q.cte;
    r64.gy = G0p * Q.cte;
    r64.h = h;
    r.alpha = (float)r64.alpha; r.sx = (float)r64.sx; r.yp = (float)(r64.gy - Q.y * h); r.h = (float)h;
    r.Ap = (float)(Q.A * 0.56418958354775628);
    r.yh = (float)(Q.y * Q.y + 0.5);
    r.y2 = (float)(2.0 * Q.y);
    r.y = (float)Q.y;
  }
  d.drec[o] = r;
  d.drec64[o] = r64;
}

extern "C" int rtx_line_prep_dt(rtx_prep* P, const rtx_lines* L, const rtx_grid* grid, int n_layers, const double* T_h,
                                const double* p_atm_h, const double* qratio_h, const double* weight_h, const double* mass_h,
                                const double* dlnsw_h, double dil_air, double dil_self, double omega_wing, double omega_wing_hw,
                                double intensity_threshold, double scale, void* stream) {
  if (!dlnsw_h) RTX_FAIL("dlnsw_h is NULL");
  if (!P || !L) RTX_FAIL("prep/lines is NULL");
  const size_t nrec = (size_t)(P->n_lines > 0 ? P->n_lines : 1) * (size_t)P->max_layers;
  // grow-only: the first call allocates, hence synchronises
  if (P->drec.reserve(nrec) || P->drec64.reserve(nrec) || P->dlnsw.reserve((size_t)L->n_species * (size_t)P->max_layers)) return 1;
  PrepArgs a;
  bool env_args = false;
  if (line_prep_grid(P, L, grid, nullptr, RTX_PREP_IN(dil_air, dil_self, nullptr, RTX_PROFILE_VOIGT), &a, &env_args)) return 1;
  if (L->n > 0) {
    hipStream_t st = (hipStream_t)stream;
    RTX_HIP(hipMemcpyAsync(P->dlnsw.get(), dlnsw_h, (size_t)L->n_species * (size_t)n_layers * sizeof(double), hipMemcpyHostToDevice, st));  // staged before returning
    PrepDTArgs d;
    d.dlnsw = P->dlnsw.get(); d.drec = P->drec.get(); d.drec64 = P->drec64.get();
    const dim3 blocks((unsigned)((L->n + 255) / 256), (unsigned)n_layers);
    if (env_args) hipLaunchKernelGGL(line_prep_dT_kernel<true>, blocks, dim3(256), 0, st, a, d);
    else hipLaunchKernelGGL(line_prep_dT_kernel<false>, blocks, dim3(256), 0, st, a, d);
    RTX_LAUNCH_CHECK();
  }
  P->dT = 1;
  return 0;
}
