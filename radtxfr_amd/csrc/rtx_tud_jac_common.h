// What the three derivative kernels of the TUD stage share: rtx_tud_jac.hip (the Jacobian J, stored), rtx_tud_vjp.hip (its
// adjoint, J^T g) and rtx_tud_jvp.hip (its tangent, J v). The limits, the description of the column and of the request
// that the kernels take, the entry points' column struct and the host code that checks it, fills the request, counts the
// workgroups and picks the instantiation, and the device functions the per-lane row factors are formed with. One copy of
// each. The column sweeps and a layer's row factors are NOT here: each kernel carries its own text of them, kept in step
// by the bit-identity tests. As device functions of this header they moved registers, occupancy or time in every kernel
// that called them (profiles/tud_deriv_refactor_isa.txt, profiles/tud_deriv_refactor_time.txt).
#pragma once
#include <math.h>
#include <string.h>

#include <type_traits>

#include "rtx_tud_common.h"

#define TUDJ_MAX_LAYERS 128
#define TUDJ_MAX_ALT 16
#define TUDJ_MAX_ANGLES 96
#define TUDJ_MAX_SPEC 16
#ifndef TUDJ_CH
#define TUDJ_CH 8  // requested layers per chunk (registers: fp64 S_l, S_l+1 and four floats each)
#endif
#ifndef TUDJ_QG
#define TUDJ_QG 8  // downwelling streams advanced together
#endif

struct TudJacArgs {
  const float* OD;       // [n_layers][ld]
  const float* ODp;      // [n_layers][ld] at T + h (windows at T), or NULL
  const float* ODm;      // [n_layers][ld] at T - h
  const float* K;        // [n_spec][n_layers][ld] OD per ppmv
  const float* tau;      // [n_alt][ld_tau] base transmittances (unused with return_od)
  float* J;              // [n_wrt][n_lay][2 n_alt + 1][ld_J]
  long long ld, ld_tau, ld_J;
  GridDev g;
  int n_layers, n_alt, n_down, n_str, return_od, with_T, n_spec, n_lay, t_pos;
  float mu, inv_2h;
  double mu_d;
  double c2l2e_over_T[TUDJ_MAX_LAYERS];  // 100 c2 log2(e) / T_k, as rtx_tud forms it
  int lay[TUDJ_MAX_LAYERS];              // requested layers, in output order
  unsigned int lbits[TUDJ_MAX_LAYERS];    // layer l: bit a = [Z_l <= zs_a] (tau mask), bit 16 + a = [l < count_a]
  int count[TUDJ_MAX_ALT];
  double str_ic[TUDJ_MAX_ANGLES];        // 1 / cos(theta_q) of the evaluated streams
  float str_w[TUDJ_MAX_ANGLES];          // omega_q = cos sin / sum(cos sin)
  float str_wc[TUDJ_MAX_ANGLES];         // omega_q / cos(theta_q)
};

// e^-y for y >= 0 given in fp64: the argument rounded once to fp32, then v_exp_f32 (|y| up to ~87 matters)
__device__ __forceinline__ float exp_neg(double y) { return __builtin_amdgcn_exp2f((float)(-y * LOG2E)); }

// 1 - e^-y, accurate to ~1e-7 relative also for a thin layer: the TUD kernels' emissivity of the transmittance's log2
__device__ __forceinline__ float one_minus_exp_neg(float y) { return emissivity(-y * (float)LOG2E); }

// B(nu, T_k) as rtx_tud evaluates it and its analytic temperature derivative: with u = c2 nu / T (t = u log2 e, the fp64
// exponent planck_f32 forms), dB/dT = B (u / T) e^u / (e^u - 1) = B (u / T) (1 + B / c1x3).
__device__ __forceinline__ void planck_dT(double c1x3, double x, double ct, float& B, float& dB) {
  B = planck_f32(c1x3, x, ct);
  // u / T = (t ln2) / T and 1/T = ct / (100 c2 log2 e)
  const double uT = x * ct * ct * (LN2 / (100.0 * RT_C2 * LOG2E));
  dB = B * (float)uT * (1.0f + B / (float)c1x3);
}

// B in fp64: only differences of neighbouring layers' B are formed from it (the recurrences of the two kernels)
__device__ __forceinline__ double planck_f64(double c1x3, double x, double ct) { return c1x3 / expm1(x * ct * LN2); }

// ---- host ---------------------------------------------------------------------------------------------
// The *_dod entry points take dOD/dT itself (rtx_voigt_sum_dt) where the others take OD at T -+ fd_step. The kernels are
// left as they are (a select on a NULL OD_minus moved the register counts of tud_vjp_kernel,
// profiles/dT_tud_resources.txt): the derivative goes in as OD_plus with fd_step = 1/2 and a library-owned array of zeros as
// OD_minus, and (D - 0) * 1 is D exactly in fp32. `count` floats of zeros on the current device (rtx_tud_jac.hip):
// grow-only, one array per device, zeroed when it is allocated and never written again.
int rtx_tud_zero_rows(size_t count, const float** out);

// The column as every entry point of the three files takes it: the 18 leading arguments of rtx_tud_jacobian
// (include/radtxfr_hip.h) and t_pos. dod: the *_dod form, where OD_plus and OD_minus both hold the caller's dOD_dT and
// fd_step is 1/2; tud_jac_setup then puts the zeros in OD_minus' place.
struct TudColumnIn {
  const float *OD, *OD_plus, *OD_minus;
  int64_t ld;
  double fd_step;
  const float* K;
  int n_spec;
  const float* tau;
  int64_t ld_tau;
  const rtx_grid* grid;
  int n_layers;
  const double* T_h;
  int n_alt;
  const uint8_t* mask_h;
  double mu;
  int n_down, n_angle, return_od, t_pos;
  bool dod;
};

// what every entry point refuses first
static inline int tud_column_check(const TudColumnIn& c) {
  if (c.dod && !c.OD_plus) RTX_FAIL("dOD_dT is NULL");
  return rtx_check_grid(c.grid);
}

// Checks everything about the column and the request that does not concern the result array, and fills `a` (J and ld_J
// stay 0). need_tau: the caller reads the base transmittances (always, for J; only with a cotangent on tau, for J^T g).
// Last, for the dod form and a shard that is not empty, the zeros: nothing before that touches the device.
static inline int tud_jac_setup(TudJacArgs& a, const TudColumnIn& c, bool need_tau, const int32_t* layers_h, int n_lay) {
  const int n_spec = c.n_spec, n_layers = c.n_layers, n_alt = c.n_alt, t_pos = c.t_pos;
  const int with_T = c.OD_plus != nullptr;
  if (!c.OD || !c.T_h || !c.mask_h || !layers_h) RTX_FAIL("a required pointer is NULL");
  if ((c.OD_plus == nullptr) != (c.OD_minus == nullptr)) RTX_FAIL("OD_plus and OD_minus are given together or not at all");
  if (with_T && !(c.fd_step > 0.0)) RTX_FAIL("fd_step=%g must be > 0", c.fd_step);
  if (n_spec < 0 || n_spec > TUDJ_MAX_SPEC) RTX_FAIL("n_spec=%d outside [0,%d]", n_spec, TUDJ_MAX_SPEC);
  if (n_spec > 0 && !c.K) RTX_FAIL("K is NULL");
  if (with_T + n_spec < 1) RTX_FAIL("nothing to differentiate (no OD_plus and n_spec = 0)");
  need_tau = need_tau && !c.return_od;
  if (need_tau && !c.tau) RTX_FAIL("tau is NULL (needed unless return_od)");
  if (n_layers < 1 || n_layers > TUDJ_MAX_LAYERS) RTX_FAIL("n_layers=%d outside [1,%d]", n_layers, TUDJ_MAX_LAYERS);
  if (n_alt < 1 || n_alt > TUDJ_MAX_ALT) RTX_FAIL("n_alt=%d outside [1,%d]", n_alt, TUDJ_MAX_ALT);
  if (c.n_angle < 1 || c.n_angle > TUDJ_MAX_ANGLES) RTX_FAIL("n_angle=%d outside [1,%d]", c.n_angle, TUDJ_MAX_ANGLES);
  if (c.n_down < 0 || c.n_down > n_layers) RTX_FAIL("n_down=%d outside [0,%d]", c.n_down, n_layers);
  if (n_lay < 1 || n_lay > TUDJ_MAX_LAYERS) RTX_FAIL("n_lay=%d outside [1,%d]", n_lay, TUDJ_MAX_LAYERS);
  if (!(c.mu >= 1.0) || !isfinite(c.mu)) RTX_FAIL("mu=%g must be finite and >= 1", c.mu);
  if (t_pos < 0 || (with_T ? t_pos > n_spec : t_pos != 0)) RTX_FAIL("t_pos=%d outside [0,%d]", t_pos, with_T ? n_spec : 0);
  if (c.ld < c.grid->n || (need_tau && c.ld_tau < c.grid->n)) RTX_FAIL("leading dimension smaller than the shard");
  memset(&a, 0, sizeof(a));
  for (int k = 0; k < n_lay; ++k) {
    if (layers_h[k] < 0 || layers_h[k] >= n_layers) RTX_FAIL("layer index %d outside [0,%d)", layers_h[k], n_layers);
    a.lay[k] = layers_h[k];
  }
  if (tud_layer_consts(c.T_h, n_layers, a.c2l2e_over_T)) return 1;
  for (int ia = 0; ia < n_alt; ++ia) {  // (rtx_tud packs the same masks per altitude; here the bits go per layer)
    int cnt = 0;
    for (int k = 0; k < n_layers; ++k)
      if (c.mask_h[(size_t)ia * n_layers + k]) { a.lbits[k] |= 1u << ia; ++cnt; }
    a.count[ia] = cnt;
    for (int k = 0; k < cnt; ++k) a.lbits[k] |= 1u << (16 + ia);
  }
  // the quadrature of rtx_tud, weights normalised (:387-388); theta = 0 has weight 0
  const TudQuadrature quad = tud_quadrature(c.n_angle);
  int ns = 0;
  for (int q = 1; q < c.n_angle; ++q) {
    const double co = cos(quad.th[q]), w = quad.w[q] / quad.wsum;
    a.str_ic[ns] = 1.0 / co;
    a.str_w[ns] = (float)w;
    a.str_wc[ns] = (float)(w / co);
    ++ns;
  }
  a.n_str = ns;
  a.OD = c.OD; a.ODp = c.OD_plus; a.ODm = c.OD_minus; a.K = c.K; a.tau = c.tau;
  a.ld = c.ld; a.ld_tau = c.ld_tau; a.g = to_dev(c.grid);
  a.n_layers = n_layers; a.n_alt = n_alt; a.n_down = c.n_down; a.return_od = c.return_od;
  a.with_T = with_T; a.n_spec = n_spec; a.n_lay = n_lay; a.t_pos = t_pos;
  a.mu = (float)c.mu; a.mu_d = c.mu; a.inv_2h = with_T ? (float)(0.5 / c.fd_step) : 0.f;
  if (c.dod && c.grid->n > 0 && rtx_tud_zero_rows((size_t)n_layers * (size_t)c.ld, &a.ODm)) return 1;
  return 0;
}

// workgroups of `per` points over the shard; a count that a launch cannot take is refused
static inline int tud_blocks(const rtx_grid* grid, int per, unsigned* blocks) {
  const long long b = (grid->n + per - 1) / per;
  if (b > 0x7fffffffLL) RTX_FAIL("grid->n=%lld: too many workgroups", (long long)grid->n);
  *blocks = (unsigned)b;
  return 0;
}

// f(TAU, LU, LD) with the three row-group flags as std::bool_constant values: the caller's generic lambda launches its
// kernel's <TAU, LU, LD> instantiation. At least one flag is set (the entry points refuse the empty selection).
template <class F>
static inline void tud_dispatch_rows(bool has_tau, bool has_Lu, bool has_Ld, F&& f) {
  using Y = std::true_type;
  using N = std::false_type;
  switch ((has_tau ? 4 : 0) | (has_Lu ? 2 : 0) | (has_Ld ? 1 : 0)) {
    case 1: f(N(), N(), Y()); break;
    case 2: f(N(), Y(), N()); break;
    case 3: f(N(), Y(), Y()); break;
    case 4: f(Y(), N(), N()); break;
    case 5: f(Y(), N(), Y()); break;
    case 6: f(Y(), Y(), N()); break;
    default: f(Y(), Y(), Y()); break;
  }
}
