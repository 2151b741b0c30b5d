// Hartmann-Tran line-sum on a line table (rtx_lines_set_ht, rtx_ht_prep, rtx_ht_sum, rtx_ht_params): the per-line block of
// absorptionCoefficient_HT, misc/hapi.py:10474-10651, for every (line, state) at once, and the windowed fp64 sum of
// PROFILE_HT over it. The profile is rtx_pcqsdhc.h (ht_setup / ht_point), the one rtx_profile_eval evaluates; the axis is
// always explicit (a device copy of the caller's sorted Omegas), so every window is the reference's bisect() on the very
// points it sums over. DESIGN.md section 4.15.
//
// Where the reference's own rows differ from one another by accident, this follows ONE row on its own: S(T)
// and Q(Tref) at 296 K whatever the previous row's lookups left in Tref; Gamma0 scaled from the Tref the n lookup leaves
// (TrefHT when n_HT is non-zero, else 296 K); Shift0's deltap (T - Tref) and NuVC's (Tref / T)^kappa with the Tref the deltap
// lookup leaves.
#include "rtx_common.h"

#include <string.h>

#include "rtx_voigt_math.h"
#include "rtx_pcqsdhc.h"

#define HT_BLOCK 256
#define HT_CHUNK 128  // records one workgroup of the sum kernel holds in LDS (128 x 160 B = 20 KiB)
#define HT_NPAR 10    // rtx_profile_eval's parameter layout
#define HT_SETS (2 + RTX_MAX_BROADENERS)
// hapi constants (misc/hapi.py:84-92, :10171, :10493)
#define H_CBOLTS 1.380648813e-16
#define H_CC 2.99792458e10
#define H_CMASSMOL 1.66053873e-27
#define H_C2 1.4388028496642257
#define H_TREF 296.0

// What the sum kernel reads of a (line, state): the profile's constants, the weighted strength and the window.
struct __attribute__((aligned(16))) HtRec {
  HtLine L;
  double WS;   // weight * S(T); 0 for a dropped line
  int lo, hi;  // axis indices [lo, hi): bisect_right(X, nu -+ OmegaWingF); lo = hi = 0 for a dropped line
};
static_assert(sizeof(HtRec) % 16 == 0, "records are staged through LDS in 16-byte pieces");

struct rtx_ht {
  long long n_lines = 0, max_points = 0;
  int max_states = 0;
  int n_states = 0;   // of the last rtx_ht_prep (0: none yet)
  long long nx = 0;
  int prepared = 0;
  double scale = 1.0;
  DevBuf<HtRec> rec;   // [max_states][n_lines]
  DevBuf<double> par;  // [max_states][n_lines][HT_NPAR]
  DevBuf<int> ic;      // [n_lines] bisect_right(X, nu): non-decreasing
  DevBuf<int> maxhw;   // [max_states] max over live lines of max(ic - lo, hi - ic) + 1
  DevBuf<double> X;    // [max_points]
  DevBuf<double> env;  // T | p | qratio | weight | mass | frac of the last prologue
};

// ---- table columns --------------------------------------------------------------------------------------------------------
extern "C" int rtx_lines_set_ht(rtx_lines* L, int n_sets, const int32_t* set_h, const double* const* cols_h) {
  if (!L) RTX_FAIL("lines is NULL");
  if (n_sets < 0 || n_sets > HT_SETS) RTX_FAIL("n_sets=%d outside [0,%d]", n_sets, HT_SETS);
  if (n_sets > 0 && (!set_h || !cols_h)) RTX_FAIL("a required pointer is NULL (set_h, cols_h)");
  for (int s = 0; s < n_sets; ++s)
    if (set_h[s] < 0 || set_h[s] >= 2 + L->n_extra)
      RTX_FAIL("HT set %d: column set %d outside [0,%d) (0 air, 1 self, 2.. rtx_lines_set_broadeners)", s, set_h[s], 2 + L->n_extra);
  L->ht_data.reset();
  L->ht_ptr.reset();
  size_t n_cols = 0;
  for (int i = 0; i < n_sets * RTX_HT_COLS; ++i) n_cols += cols_h[i] != nullptr;
  if (n_cols == 0 || L->n == 0) return 0;
  const size_t n = (size_t)L->n;
  DevBuf<double> data;
  DevBuf<const double*> ptr;
  if (data.reserve(n_cols * n)) return 1;
  std::vector<const double*> tab((size_t)HT_SETS * RTX_HT_COLS, nullptr);
  size_t c = 0;
  for (int s = 0; s < n_sets; ++s)
    for (int j = 0; j < RTX_HT_COLS; ++j) {
      const double* h = cols_h[(size_t)s * RTX_HT_COLS + j];
      tab[(size_t)set_h[s] * RTX_HT_COLS + j] = nullptr;
      if (!h) continue;
      double* d = data.get() + c++ * n;
      if (rtx_dev_h2d(d, h, n * sizeof(double))) return 1;
      tab[(size_t)set_h[s] * RTX_HT_COLS + j] = d;
    }
  if (ptr.upload(tab.data(), tab.size())) return 1;
  L->ht_data = std::move(data);
  L->ht_ptr = std::move(ptr);
  return 0;
}

// ---- prologue ----------------------------------------------------------------------------------------------------------------
struct HtPrepArgs {
  const double *nu, *sw, *elower, *zn, *gamma_air, *gamma_self, *n_air, *n_self, *delta_air, *deltap_air, *delta_self, *deltap_self;
  const double *sd_air, *sd_self;
  const double *x_gamma, *x_n, *x_delta, *x_deltap, *x_sd;  // extra sets [n_extra][n], fallbacks applied (rtx_lines_set_broadeners)
  const double* const* ht;                                    // [HT_SETS][RTX_HT_COLS] device pointers, or NULL: no HT column
  const int* species;
  long long n_lines;
  int n_states, n_species;
  const double *T, *p, *qratio, *weight, *mass, *frac;  // device copies
  int n_dil;
  int dil_idx[RTX_MAX_DILUENTS];
  double omega_wing, omega_wing_hw, thresh;
  const double* X;
  long long nx;
  HtRec* rec;
  double* par;
  int* ic;
  int* maxhw;
};

// bisect.bisect (= bisect_right) of v on the axis: the number of points <= v
__device__ long long ht_bisect(const double* __restrict__ X, long long nx, double v) {
  long long lo = 0, hi = nx;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (v < X[mid]) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// The Voigt-style columns of set c (0 air, 1 self, 2 + j) with the reference's fallbacks (:10513-10538, :10556-10577, :10591):
// an absent gamma / delta / deltap / SD is 0, an absent n is n_air, and so is a self n of 0
struct HtVoigtCols {
  double g, n, d, dp, sd;
};
__device__ __forceinline__ HtVoigtCols ht_voigt_cols(const HtPrepArgs& a, int c, long long l) {
  HtVoigtCols r;
  if (c == 0) {
    r.g = a.gamma_air[l]; r.n = a.n_air[l]; r.d = a.delta_air[l];
    r.dp = a.deltap_air ? a.deltap_air[l] : 0.0;
    r.sd = a.sd_air ? a.sd_air[l] : 0.0;
  } else if (c == 1) {
    double ns = a.n_self ? a.n_self[l] : a.n_air[l];
    if (a.n_self && ns == 0.0) ns = a.n_air[l];
    r.g = a.gamma_self[l]; r.n = ns;
    r.d = a.delta_self ? a.delta_self[l] : 0.0;
    r.dp = a.deltap_self ? a.deltap_self[l] : 0.0;
    r.sd = a.sd_self ? a.sd_self[l] : 0.0;
  } else {
    const size_t o = (size_t)(c - 2) * (size_t)a.n_lines + (size_t)l;
    r.g = a.x_gamma[o]; r.n = a.x_n[o]; r.d = a.x_delta[o]; r.dp = a.x_deltap[o]; r.sd = a.x_sd[o];
  }
  return r;
}

// One thread per (line, state): misc/hapi.py:10474-10647 for that row, then the profile's constants (ht_setup).
__global__ __launch_bounds__(HT_BLOCK) void ht_prep_kernel(HtPrepArgs a) {
  const long long l = (long long)blockIdx.x * HT_BLOCK + threadIdx.x;
  const int k = blockIdx.y;
  if (l >= a.n_lines) return;
  const double T = a.T[k], p = a.p[k];
  const double nu = a.nu[l];
  const int sp = a.species[l];
  const double w = a.weight[(size_t)sp * a.n_states + k];
  // TrefHT (:10394-10398): a temperature in none of the ranges leaves the loop's last value
  const int b = (T >= 0.0 && T < 100.0) ? 0 : (T >= 100.0 && T < 200.0) ? 1 : (T >= 200.0 && T < 400.0) ? 2 : 3;
  const double TrefHT = b == 0 ? 50.0 : b == 1 ? 150.0 : b == 2 ? 296.0 : 700.0;
  // S(T) from 296 K (:10169-10175; SigmaTref / SigmaT = qratio)
  const double ch = exp(-H_C2 * a.elower[l] / T) * (1.0 - exp(-H_C2 * nu / T));
  const double S = a.sw[l] * a.qratio[(size_t)sp * a.n_states + k] * ch / a.zn[l];
  const bool dropped = !(w != 0.0) || (S < a.thresh);
  // GammaD (:10493-10495)
  const double m = a.mass[sp] * H_CMASSMOL * 1000.0;
  const double GammaD = sqrt(2.0 * H_CBOLTS * T * log(2.0) / m / (H_CC * H_CC)) * nu;
  double Gamma0 = 0.0, Shift0 = 0.0, Gamma2 = 0.0, Shift2 = 0.0, NuVC = 0.0;
  cd EtaNumer = {0.0, 0.0};
  for (int d = 0; d < a.n_dil; ++d) {
    const double abun = a.frac[((size_t)d * a.n_species + sp) * a.n_states + k];
    const int c = a.dil_idx[d];
    const HtVoigtCols q = ht_voigt_cols(a, c, l);
    const double* const* hc = a.ht ? a.ht + (size_t)c * RTX_HT_COLS : nullptr;
    auto ht = [&](int slot) -> double { return hc && hc[slot] ? hc[slot][l] : 0.0; };  // absent and 0 behave the same
    double Gamma0DB = ht(6 * b + 0);
    if (Gamma0DB == 0.0) Gamma0DB = q.g;
    double n = ht(6 * b + 1), Tref = TrefHT;
    if (n == 0.0) { n = q.n; Tref = H_TREF; }
    const double Gamma0T = Gamma0DB * p / 1.0 * pow(Tref / T, n);  // :10184
    Gamma0 += abun * Gamma0T;
    double Shift0DB = ht(6 * b + 3);
    if (Shift0DB == 0.0) Shift0DB = q.d;
    double deltap = ht(6 * b + 4);
    Tref = TrefHT;
    if (deltap == 0.0) { deltap = q.dp; Tref = H_TREF; }
    const double Shift0T = (Shift0DB + deltap * (T - Tref)) * p / 1.0;  // :10581
    Shift0 += abun * Shift0T;
    double Gamma2DB = ht(6 * b + 2);
    if (Gamma2DB == 0.0) Gamma2DB = q.sd * Gamma0DB;  // :10592
    Gamma2 += abun * (Gamma2DB * (p / 1.0));
    Shift2 += abun * (ht(6 * b + 5) * p / 1.0);
    NuVC += abun * (ht(24) * pow(Tref / T, ht(25)) * p);  // :10629, the Tref of the deltap lookup
    const double ea = ht(26) * abun;
    EtaNumer.r += ea * Gamma0T;
    EtaNumer.i += ea * Shift0T;
  }
  const cd Eta = cdiv_lib(EtaNumer, cd{Gamma0, Shift0});
  // OmegaWingF and the window (:10644-10647), centred on the unshifted nu
  const double W = fmax(a.omega_wing, fmax(a.omega_wing_hw * Gamma0, a.omega_wing_hw * GammaD));
  long long lo = ht_bisect(a.X, a.nx, nu - W), hi = ht_bisect(a.X, a.nx, nu + W);
  if (dropped || hi <= lo) { lo = 0; hi = 0; }
  const long long ic = ht_bisect(a.X, a.nx, nu);
  if (k == 0) a.ic[l] = (int)ic;
  const size_t o = (size_t)k * (size_t)a.n_lines + (size_t)l;
  double* __restrict__ par = a.par + o * HT_NPAR;
  par[0] = nu; par[1] = GammaD; par[2] = Gamma0; par[3] = Gamma2; par[4] = Shift0; par[5] = Shift2; par[6] = NuVC;
  par[7] = Eta.r; par[8] = Eta.i; par[9] = 0.0;
  HtRec* __restrict__ r = a.rec + o;
  ht_setup(par, &r->L);
  r->WS = dropped ? 0.0 : w * S;
  r->lo = (int)lo;
  r->hi = (int)hi;
  if (hi > lo) {
    const long long hw = (ic - lo > hi - ic ? ic - lo : hi - ic) + 1;
    atomicMax(&a.maxhw[k], (int)hw);
  }
}

// ---- the sum: a gather, one workgroup per 256 consecutive axis points of one state ------------------------------------------
struct HtSumArgs {
  const HtRec* rec;
  const int* ic;
  const int* maxhw;
  const double* X;
  long long n_lines, nx;
  float* out32;
  double* out64;
  long long ld;
  double scale;
};

// Candidates: the lines whose centre index lies within the state's largest half-width of the block (binary search on the
// sorted ic). Their records go through LDS HT_CHUNK at a time; a line whose window misses the block is skipped on a uniform
// branch, and each thread tests its own index. acc = acc + WS Re LS in line order, one association: a point's value depends
// on neither the launch shape nor the rest of the axis.
__global__ __launch_bounds__(HT_BLOCK) void ht_sum_kernel(HtSumArgs a) {
  __shared__ int s_rng[2];
  __shared__ HtRec s_rec[HT_CHUNK];
  const int k = blockIdx.y;
  const long long i0 = (long long)blockIdx.x * HT_BLOCK;
  if (threadIdx.x == 0) {
    const long long hw = a.maxhw[k];
    const long long lo_v = i0 - hw, hi_v = i0 + (HT_BLOCK - 1) + hw;
    long long lo = 0, hi = a.n_lines;
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if ((long long)a.ic[mid] < lo_v) lo = mid + 1; else hi = mid;
    }
    const long long first = lo;
    hi = a.n_lines;
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if ((long long)a.ic[mid] <= hi_v) lo = mid + 1; else hi = mid;
    }
    s_rng[0] = (int)first;
    s_rng[1] = (int)(hw > 0 ? lo : first);  // no live line in this state: nothing to do
  }
  __syncthreads();
  const int first = s_rng[0], last = s_rng[1];
  const long long i = i0 + threadIdx.x;
  const double s = i < a.nx ? a.X[i] : 0.0;
  const long long b_lo = i0, b_hi = i0 + HT_BLOCK < a.nx ? i0 + HT_BLOCK : a.nx;
  const HtRec* __restrict__ rec = a.rec + (size_t)k * (size_t)a.n_lines;
  double acc = 0.0;
  for (int base = first; base < last; base += HT_CHUNK) {
    const int m = last - base < HT_CHUNK ? last - base : HT_CHUNK;
    __syncthreads();  // the previous chunk is no longer read
    {
      const uint4* __restrict__ src = reinterpret_cast<const uint4*>(rec + base);
      uint4* dst = reinterpret_cast<uint4*>(s_rec);
      const int cnt = m * (int)(sizeof(HtRec) / 16);
      for (int t = threadIdx.x; t < cnt; t += HT_BLOCK) dst[t] = src[t];
    }
    __syncthreads();
    for (int j = 0; j < m; ++j) {
      const long long lo = s_rec[j].lo, hi = s_rec[j].hi;  // a dropped line has lo = hi = 0
      if (hi <= b_lo || lo >= b_hi) continue;              // the whole block lies outside this line's window (uniform branch)
      if (i >= lo && i < hi) acc = acc + s_rec[j].WS * ht_point(&s_rec[j].L, s).r;
    }
  }
  if (i < a.nx) {
    const size_t o = (size_t)k * (size_t)a.ld + (size_t)i;
    if (a.out64) a.out64[o] = acc;
    if (a.out32) a.out32[o] = (float)(acc * a.scale);
  }
}

// strengths and windows of one state's records, for rtx_ht_params
__global__ __launch_bounds__(HT_BLOCK) void ht_unpack_kernel(const HtRec* __restrict__ rec, long long n, double* __restrict__ strength,
                                                             int32_t* __restrict__ window) {
  const long long l = (long long)blockIdx.x * HT_BLOCK + threadIdx.x;
  if (l >= n) return;
  if (strength) strength[l] = rec[l].WS;
  if (window) {
    window[2 * l] = rec[l].lo;
    window[2 * l + 1] = rec[l].hi;
  }
}

// ---- entry points -------------------------------------------------------------------------------------------------------------
extern "C" int rtx_ht_free(rtx_ht* H) {
  delete H;
  return 0;
}

extern "C" int rtx_ht_create(int64_t n_lines, int max_states, int64_t max_points, rtx_ht** out) {
  if (!out) RTX_FAIL("out is NULL");
  *out = nullptr;
  if (n_lines < 0 || n_lines > 2000000000LL) RTX_FAIL("n_lines=%lld outside [0,2e9]", (long long)n_lines);
  if (max_states < 1 || max_states > 4096) RTX_FAIL("max_states=%d outside [1,4096]", max_states);
  if (max_points < 1 || max_points > 2000000000LL) RTX_FAIL("max_points=%lld outside [1,2e9]", (long long)max_points);
  rtx_ht* H = new rtx_ht();
  H->n_lines = n_lines;
  H->max_states = max_states;
  H->max_points = max_points;
  *out = H;  // device memory is taken by the first rtx_ht_prep that has work to do
  return 0;
}

extern "C" int rtx_ht_prep(rtx_ht* H, const rtx_lines* L, const double* X_h, int64_t nx, int n_states, const double* T_h,
                           const double* p_atm_h, const double* qratio_h, const double* weight_h, const double* mass_h, int n_dil,
                           const int32_t* dil_h, const double* frac_h, double omega_wing, double omega_wing_hw,
                           double intensity_threshold, double scale, void* stream) {
  if (!H) RTX_FAIL("a required pointer is NULL (ht)");
  if (nx < 0) RTX_FAIL("nx=%lld", (long long)nx);
  if (nx > H->max_points) RTX_FAIL("nx=%lld points, the object was created for %lld", (long long)nx, H->max_points);
  if (n_states < 1 || n_states > H->max_states) RTX_FAIL("n_states=%d outside [1,%d]", n_states, H->max_states);
  if (n_dil < 0 || n_dil > RTX_MAX_DILUENTS) RTX_FAIL("n_dil=%d outside [0,%d]", n_dil, RTX_MAX_DILUENTS);
  if (!L || !T_h || !p_atm_h || !qratio_h || !weight_h || !mass_h || (nx > 0 && !X_h) || (n_dil > 0 && (!dil_h || !frac_h)))
    RTX_FAIL("a required pointer is NULL (lines, X_h, T_h, p_atm_h, qratio_h, weight_h, mass_h, dil_h, frac_h)");
  if (H->n_lines != L->n) RTX_FAIL("the object was created for %lld lines, the table has %lld", H->n_lines, L->n);
  if (!(scale > 0.0)) RTX_FAIL("scale must be > 0");
  for (int d = 0; d < n_dil; ++d)
    if (dil_h[d] < 0 || dil_h[d] >= 2 + L->n_extra)
      RTX_FAIL("diluent %d: column set %d outside [0,%d) (0 air, 1 self, 2.. rtx_lines_set_broadeners)", d, dil_h[d], 2 + L->n_extra);
  for (int k = 0; k < n_states; ++k)
    if (!(T_h[k] > 0.0) || !(p_atm_h[k] >= 0.0)) RTX_FAIL("state %d: T=%g p=%g not physical", k, T_h[k], p_atm_h[k]);
  for (int64_t i = 0; i < nx; ++i) {
    if (!isfinite(X_h[i])) RTX_FAIL("axis point %lld is not finite", (long long)i);
    if (i > 0 && X_h[i] < X_h[i - 1]) RTX_FAIL("axis must be non-decreasing (point %lld)", (long long)i);
  }
  H->n_states = n_states;
  H->nx = nx;
  H->scale = scale;
  H->prepared = 1;
  if (L->n == 0 || nx == 0) return 0;  // nothing to do: no launch
  hipStream_t st = (hipStream_t)stream;
  const size_t n1 = (size_t)L->n, nrec = n1 * (size_t)H->max_states, ns = (size_t)L->n_species;
  const size_t nT = (size_t)n_states, nQ = ns * nT, nF = (size_t)n_dil * nQ;
  const size_t env_cap = (size_t)H->max_states * (2 + 2 * ns + (size_t)RTX_MAX_DILUENTS * ns) + ns;
  if (H->rec.reserve(nrec) || H->par.reserve(nrec * HT_NPAR) || H->ic.reserve(n1) || H->maxhw.reserve((size_t)H->max_states) ||
      H->X.reserve((size_t)H->max_points) || H->env.reserve(env_cap))
    return 1;
  std::vector<double> env(2 * nT + 2 * nQ + ns + nF);
  double* e = env.data();
  memcpy(e, T_h, nT * sizeof(double));
  memcpy(e + nT, p_atm_h, nT * sizeof(double));
  memcpy(e + 2 * nT, qratio_h, nQ * sizeof(double));
  memcpy(e + 2 * nT + nQ, weight_h, nQ * sizeof(double));
  memcpy(e + 2 * nT + 2 * nQ, mass_h, ns * sizeof(double));
  if (nF) memcpy(e + 2 * nT + 2 * nQ + ns, frac_h, nF * sizeof(double));
  // pageable-source async copies are staged by the runtime before returning: the caller may reuse its arrays
  RTX_HIP(hipMemcpyAsync(H->env.get(), e, env.size() * sizeof(double), hipMemcpyHostToDevice, st));
  RTX_HIP(hipMemcpyAsync(H->X.get(), X_h, (size_t)nx * sizeof(double), hipMemcpyHostToDevice, st));
  RTX_HIP(hipMemsetAsync(H->maxhw.get(), 0, (size_t)H->max_states * sizeof(int), st));
  HtPrepArgs a;
  a.nu = L->nu.get(); a.sw = L->sw.get(); a.elower = L->elower.get(); a.zn = L->zn.get();
  a.gamma_air = L->gamma_air.get(); a.gamma_self = L->gamma_self.get(); a.n_air = L->n_air.get(); a.n_self = L->n_self.get();
  a.delta_air = L->delta_air.get(); a.deltap_air = L->deltap_air.get(); a.delta_self = L->delta_self.get();
  a.deltap_self = L->deltap_self.get(); a.sd_air = L->sd_air.get(); a.sd_self = L->sd_self.get();
  a.x_gamma = L->x_gamma.get(); a.x_n = L->x_n.get(); a.x_delta = L->x_delta.get(); a.x_deltap = L->x_deltap.get(); a.x_sd = L->x_sd.get();
  a.ht = L->ht_ptr.get();
  a.species = L->species.get();
  a.n_lines = L->n; a.n_states = n_states; a.n_species = L->n_species;
  const double* d = H->env.get();
  a.T = d; a.p = d + nT; a.qratio = d + 2 * nT; a.weight = d + 2 * nT + nQ; a.mass = d + 2 * nT + 2 * nQ;
  a.frac = d + 2 * nT + 2 * nQ + ns;
  a.n_dil = n_dil;
  for (int i = 0; i < RTX_MAX_DILUENTS; ++i) a.dil_idx[i] = i < n_dil ? dil_h[i] : 0;
  a.omega_wing = omega_wing; a.omega_wing_hw = omega_wing_hw; a.thresh = intensity_threshold;
  a.X = H->X.get(); a.nx = nx;
  a.rec = H->rec.get(); a.par = H->par.get(); a.ic = H->ic.get(); a.maxhw = H->maxhw.get();
  hipLaunchKernelGGL(ht_prep_kernel, dim3((unsigned)((L->n + HT_BLOCK - 1) / HT_BLOCK), (unsigned)n_states), dim3(HT_BLOCK), 0, st, a);
  RTX_LAUNCH_CHECK();
  return 0;
}

extern "C" int rtx_ht_sum(const rtx_ht* H, int n_states, float* out_f32, double* out_f64, int64_t ld, void* stream) {
  if (!H) RTX_FAIL("a required pointer is NULL (ht)");
  if (!out_f32 && !out_f64) RTX_FAIL("a required pointer is NULL (no output given)");
  if (!H->prepared) RTX_FAIL("rtx_ht_prep has not been run on this object");
  if (n_states < 1 || n_states > H->n_states) RTX_FAIL("n_states=%d, the prologue was run for %d", n_states, H->n_states);
  if (ld < H->nx) RTX_FAIL("ld=%lld smaller than n=%lld", (long long)ld, H->nx);
  if (H->nx == 0) return 0;  // nothing to do: no launch
  hipStream_t st = (hipStream_t)stream;
  if (H->n_lines == 0) {  // no line: zeros, row by row (ld may exceed n)
    for (int k = 0; k < n_states; ++k) {
      if (out_f64) RTX_HIP(hipMemsetAsync(out_f64 + (size_t)k * (size_t)ld, 0, (size_t)H->nx * sizeof(double), st));
      if (out_f32) RTX_HIP(hipMemsetAsync(out_f32 + (size_t)k * (size_t)ld, 0, (size_t)H->nx * sizeof(float), st));
    }
    return 0;
  }
  HtSumArgs a;
  a.rec = H->rec.get(); a.ic = H->ic.get(); a.maxhw = H->maxhw.get(); a.X = H->X.get();
  a.n_lines = H->n_lines; a.nx = H->nx;
  a.out32 = out_f32; a.out64 = out_f64; a.ld = ld; a.scale = H->scale;
  hipLaunchKernelGGL(ht_sum_kernel, dim3((unsigned)((H->nx + HT_BLOCK - 1) / HT_BLOCK), (unsigned)n_states), dim3(HT_BLOCK), 0, st, a);
  RTX_LAUNCH_CHECK();
  return 0;
}

extern "C" int rtx_ht_params(const rtx_ht* H, int state, double* params, double* strength, int32_t* window, void* stream) {
  if (!H) RTX_FAIL("a required pointer is NULL (ht)");
  if (!H->prepared) RTX_FAIL("rtx_ht_prep has not been run on this object");
  if (state < 0 || state >= H->n_states) RTX_FAIL("state=%d, the prologue was run for %d", state, H->n_states);
  if (H->n_lines == 0 || H->nx == 0) return 0;  // the prologue had nothing to do: nothing is written
  hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)H->n_lines, o = (size_t)state * n;
  if (params) RTX_HIP(hipMemcpyAsync(params, H->par.get() + o * HT_NPAR, n * HT_NPAR * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (strength || window) {
    hipLaunchKernelGGL(ht_unpack_kernel, dim3((unsigned)((n + HT_BLOCK - 1) / HT_BLOCK)), dim3(HT_BLOCK), 0, st, H->rec.get() + o,
                       (long long)n, strength, window);
    RTX_LAUNCH_CHECK();
  }
  return 0;
}
