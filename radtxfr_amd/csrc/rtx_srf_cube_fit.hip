// Per-pixel fit of temperature and fractions to a measured HSI cube (include/radtxfr_hip.h, rtx_srf_pixel_cube_normal and
// rtx_srf_pixel_cube_fit): the atmosphere (N, C, tab = G) and each pixel's endmember indices are fixed, the
// unknowns of pixel p are u = (T, f_1 .. f_nMix), the model is rtx_srf_pixel_cube's
//   y_b(u) = ( C_b + sum_m f_m sum_q l_q(T) G[k_m][q][b] ) / N_b
// and a band COUNTS when it is live (N_b > 0) and its weight w_b > 0 (wgt == NULL: 1). With r_b = y_b - meas[b][p],
//   cost = sum_b w_b r_b^2,   grad = J^T W r,   H = J^T W J (lower triangle, rows: H_00, H_10, H_11, H_20, ...),
//   J_b0 = sum_m f_m t'_m / N_b,   J_bm = t_m / N_b,   t_m = sum_q l_q G[k_m][q][b],   t'_m = sum_q l'_q G[k_m][q][b].
//
// LANE = PIXEL. A workgroup of SCF_PB = 64 threads (one wave) owns 64 pixels; every sum of a pixel lives in its lane's
// registers (1 + (1 + nMix) + (1 + nMix)(2 + nMix) / 2 fp64 values per evaluation), nothing crosses lanes, no atomics, no
// workspace. The band sum runs over THE BANDS ASCENDING IN ONE LANE, for every table placement. meas[b][64 pixels] is one
// 256-byte row per band. The table slice of a block of 64 bands sits in LDS when nEnd * Q <= SCF_TAB_LDS (as the three
// sibling kernels decide it), laid out [band][endmember][node] so that a lane reads its endmember's Q nodes in 16-byte
// pieces; otherwise every lane reads its entries from global memory. The kernels are templates on Q and nMix, fully
// unrolled: H is never indexed dynamically.
//
// One evaluation (scf_eval), per counting band, fp32 then fp64:
//   w_q = (float)l_q, w'_q = (float)l'_q from srf_cube_weight (the adjoint's code: l_q has the forward's bits)
//   t_m = fmaf(w_q, G, t_m), t'_m = fmaf(w'_q, G, t'_m), q ascending;  s = fmaf(f_m, t_m, s), m ascending
//   y = (C_b + s) / N_b                                              (fp32: the forward's bits)
//   r = (double)y - (double)meas;  invN = 1 / (double)N_b
//   j_0 = invN * S, S = fma((double)f_m, (double)t'_m, S) m ascending;  j_m = invN * (double)t_m
//   wr = w r;  cost = fma(wr, r, cost);  grad_i = fma(j_i, wr, grad_i);  H_ij = fma(w j_i, j_j, H_ij), i >= j
// Damped step (scf_solve): A = H with A_ii = fma(lambda, H_ii, H_ii); Cholesky A = L L^T by columns,
//   d = A_jj; d = fma(-L_jk, L_jk, d) k ascending; a pivot d that is not finite or not > 0: singular, the step NaN;
//   L_jj = sqrt(d);  L_ij = (A_ij - sum_k L_ik L_jk) / L_jj, the sum by fma(-L_ik, L_jk, .) k ascending;
//   z_i = (-grad_i - sum_{k<i} L_ik z_k) / L_ii, i ascending;  step_i = (z_i - sum_{k>i} L_ki step_k) / L_ii, i descending.
// The fit (scf_fit_kernel) is one loop with one call of scf_eval in it: first the start (the given point, or the node
// scan: per node q an evaluation at (T_q, 0), the fraction block's solve, an evaluation at (T_q, f_q)), then the
// Levenberg-Marquardt trials. The loop is uniform over the wave; a lane that has stopped carries a status and rides along.
// rtx_srf_pixel_cube_normal is one evaluation and one solve by the same device functions: a host loop over it has the
// fit's bits.
#define SCF_PB 64        // pixels per workgroup: one wave
#define SCF_TAB_LDS 128  // nEnd * Q up to which the table slice lives in LDS (rtx_srf_cube.hip's SC_TAB_LDS)
#include "rtx_srf_cube_fit_common.h"  // ScfArgs, ScfSums, scf_eval, scf_solve, scf_trial, scf_front: shared with rtx_srf_cube_fit_box.hip

template <int Q, int NM>
__global__ __launch_bounds__(SCF_PB) void scf_normal_kernel(ScfArgs a) {
  extern __shared__ float4 s_dyn[];
  constexpr int NU = NM + 1, NH = ScfSums<NM>::NH;
  const long long p_own = (long long)blockIdx.x * SCF_PB + threadIdx.x;
  const long long p = min(p_own, a.nPix - 1);  // past the end: the last pixel again, never stored
  const double T = a.T_in[p];
  const bool ok = T >= a.T_lo && T <= a.T_hi;  // false for NaN
  float f[NM];
  int k[NM];
#pragma unroll
  for (int m = 0; m < NM; ++m) {
    f[m] = a.frac_in[p * NM + m];
    k[m] = min(max(a.kidx[p * NM + m], 0), a.nEnd - 1);  // clamped as the forward clamps it
  }
  ScfSums<NM> o;
  scf_eval<Q, NM>(a, reinterpret_cast<float*>(s_dyn), p, T, f, k, o);
  if (p_own >= a.nPix) return;
  const double nan = __builtin_nan("");
  a.cost[p] = ok ? o.c : nan;
  if (a.grad) {
#pragma unroll
    for (int i = 0; i < NU; ++i) a.grad[p * NU + i] = ok ? o.g[i] : nan;
  }
  if (a.hess) {
#pragma unroll
    for (int i = 0; i < NH; ++i) a.hess[p * NH + i] = ok ? o.H[i] : nan;
  }
  if (a.step) {
    double d[NU];
    scf_solve<NM, 0, NU>(o, a.lambda ? a.lambda[p] : 0.0, d);
#pragma unroll
    for (int i = 0; i < NU; ++i) a.step[p * NU + i] = ok ? d[i] : nan;
  }
}

template <int Q, int NM>
__global__ __launch_bounds__(SCF_PB) void scf_fit_kernel(ScfArgs a) {
  extern __shared__ float4 s_dyn[];
  constexpr int NU = NM + 1, NH = ScfSums<NM>::NH;
  const long long p_own = (long long)blockIdx.x * SCF_PB + threadIdx.x;
  const long long p = min(p_own, a.nPix - 1);
  const bool given = a.given != 0;
  const int n_pre = given ? 1 : 2 * Q;  // evaluations of the start
  int k[NM];
  float f[NM], ft[NM];
  double T = a.T_lo, Tt = a.T_lo;
  int status = p_own < a.nPix ? -1 : 0;  // -1: running
#pragma unroll
  for (int m = 0; m < NM; ++m) {
    k[m] = min(max(a.kidx[p * NM + m], 0), a.nEnd - 1);
    f[m] = ft[m] = 0.f;
  }
  if (given) {
    T = Tt = a.Tpix[p];
    bool fin = T >= a.T_lo && T <= a.T_hi;
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      f[m] = ft[m] = a.frac[p * NM + m];
      fin = fin && fabsf(f[m]) <= 3.40282346638528859812e38f;  // false for NaN and infinity
    }
    if (!fin && status < 0) status = 2;
    if (!fin) { T = Tt = a.T_lo; }  // a stand-in: the lane rides along, nothing of it is kept
  }
  ScfSums<NM> cur, tr;
  cur.c = __builtin_inf();
#pragma unroll
  for (int i = 0; i < NU; ++i) cur.g[i] = 0.0;
#pragma unroll
  for (int i = 0; i < NH; ++i) cur.H[i] = 0.0;
  double lam = a.lambda0;
  int n_iter = 0;
  bool node_ok = false;
  for (int e = 0;; ++e) {
    if (e < n_pre) {
      if (!given) {
        const int q = e >> 1;
#pragma unroll
        for (int r = 0; r < Q; ++r)
          if (r == q) Tt = a.Tn[r];
        if (!(e & 1)) {
#pragma unroll
          for (int m = 0; m < NM; ++m) ft[m] = 0.f;
        }
      }
    } else if (status < 0) {
      if (cur.c == 0.0) status = 0;
      else if (n_iter >= a.max_iter) status = 1;
      else {
        double d[NU];
        if (scf_solve<NM, 0, NU>(cur, lam, d)) scf_trial<NM>(a, T, f, d, Tt, ft);
        else status = 3;
      }
    }
    if (!__syncthreads_or(e < n_pre || status < 0)) break;
    scf_eval<Q, NM>(a, reinterpret_cast<float*>(s_dyn), p, Tt, ft, k, tr);
    if (e < n_pre) {
      if (given) {
        cur = tr;
      } else if (!(e & 1)) {  // the fraction block alone, undamped, from the evaluation at f = 0
        double d[NM];
        node_ok = scf_solve<NM, 1, NM>(tr, 0.0, d);
#pragma unroll
        for (int m = 0; m < NM; ++m) ft[m] = (float)d[m];
      } else if (node_ok && tr.c < cur.c) {  // strictly smaller: the first node wins a tie; NaN and infinity never win
        cur = tr;
        T = Tt;
#pragma unroll
        for (int m = 0; m < NM; ++m) f[m] = ft[m];
      }
      if (e == n_pre - 1 && status < 0 && !(fabs(cur.c) <= 1.79769313486231570815e308)) status = 3;  // no finite cost to start from
    } else if (status < 0) {
      ++n_iter;
      if (tr.c < cur.c) {  // false for a NaN cost
        const double was = cur.c;
        cur = tr;
        T = Tt;
#pragma unroll
        for (int m = 0; m < NM; ++m) f[m] = ft[m];
        lam = fmax(0.1 * lam, SCF_LAM_MIN);
        if (was - cur.c < a.ftol * was) status = 0;
      } else {
        lam = fmin(10.0 * lam, SCF_LAM_MAX);
        if (lam >= SCF_LAM_MAX) status = 0;
      }
    }
  }
  if (p_own >= a.nPix) return;
  const bool good = status < 2;
  const double nan = __builtin_nan("");
  a.Tpix[p] = good ? T : nan;
#pragma unroll
  for (int m = 0; m < NM; ++m) a.frac[p * NM + m] = good ? f[m] : __builtin_nanf("");
  a.cost[p] = good ? cur.c : nan;
  a.n_iter[p] = n_iter;
  a.status[p] = status;
  if (a.hess) {
#pragma unroll
    for (int i = 0; i < NH; ++i) a.hess[p * NH + i] = good ? cur.H[i] : nan;
  }
}

template <int Q, int NM>
static void launch_scf(const ScfArgs& a, bool fit, hipStream_t st) {
  const dim3 grid((unsigned)((a.nPix + SCF_PB - 1) / SCF_PB));
  const size_t lds = (size_t)a.stride * 64 * sizeof(float);
  if (fit) hipLaunchKernelGGL((scf_fit_kernel<Q, NM>), grid, dim3(SCF_PB), lds, st, a);
  else hipLaunchKernelGGL((scf_normal_kernel<Q, NM>), grid, dim3(SCF_PB), lds, st, a);
}

template <int Q>
static void launch_scf_mix(const ScfArgs& a, int nMix, bool fit, hipStream_t st) {
  switch (nMix) {
    case 1: launch_scf<Q, 1>(a, fit, st); break;
    case 2: launch_scf<Q, 2>(a, fit, st); break;
    case 3: launch_scf<Q, 3>(a, fit, st); break;
    default: launch_scf<Q, 4>(a, fit, st); break;
  }
}

static void scf_launch(const ScfArgs& a, int Q, int nMix, bool fit, hipStream_t st) {
  switch (Q) {
    case 1: launch_scf_mix<1>(a, nMix, fit, st); break;
    case 2: launch_scf_mix<2>(a, nMix, fit, st); break;
    case 3: launch_scf_mix<3>(a, nMix, fit, st); break;
    case 4: launch_scf_mix<4>(a, nMix, fit, st); break;
    case 5: launch_scf_mix<5>(a, nMix, fit, st); break;
    case 6: launch_scf_mix<6>(a, nMix, fit, st); break;
    case 7: launch_scf_mix<7>(a, nMix, fit, st); break;
    default: launch_scf_mix<8>(a, nMix, fit, st); break;
  }
}

extern "C" int rtx_srf_pixel_cube_fit_max_mix(void) { return SCF_MIX_MAX; }
extern "C" int rtx_srf_pixel_cube_fit_max_iter(void) { return SCF_ITER_MAX; }

extern "C" int rtx_srf_pixel_cube_normal(int nB, int Q, const double* T_node_h, const float* N, const float* C, const float* tab, int nEnd,
                                         int64_t nPix, int nMix, const int32_t* kidx, const float* frac, const double* Tpix, const float* meas,
                                         const float* wgt, const double* lambda, double* cost, double* grad, double* hess, double* step,
                                         void* stream, unsigned flags) {
  if (flags != 0) RTX_FAIL("rtx_srf_pixel_cube_normal: flags=%u, none is defined", flags);
  ScfArgs a;
  if (scf_front("rtx_srf_pixel_cube_normal", a, nB, Q, T_node_h, nEnd, nPix, nMix)) return 1;
  if (!meas || !cost) RTX_FAIL("rtx_srf_pixel_cube_normal: a required pointer is NULL (meas, cost)");
  if (nB == 0 || nPix == 0) return 0;
  if (!N || !C || !tab || !kidx || !frac || !Tpix) RTX_FAIL("rtx_srf_pixel_cube_normal: a required pointer is NULL");
  a.N = N; a.C = C; a.tab = tab; a.kidx = kidx; a.meas = meas; a.wgt = wgt;
  a.frac_in = frac; a.T_in = Tpix; a.lambda = lambda;
  a.cost = cost; a.grad = grad; a.hess = hess; a.step = step;
  scf_launch(a, Q, nMix, false, (hipStream_t)stream);
  RTX_LAUNCH_CHECK();
  return 0;
}

extern "C" int rtx_srf_pixel_cube_fit(int nB, int Q, const double* T_node_h, const float* N, const float* C, const float* tab, int nEnd,
                                      int64_t nPix, int nMix, const int32_t* kidx, const float* meas, const float* wgt, float* frac, double* Tpix,
                                      int max_iter, double lambda0, double ftol, double* cost, int32_t* n_iter, int32_t* status, double* hess,
                                      void* stream, unsigned flags) {
  if (flags & ~(unsigned)RTX_FIT_START_GIVEN) RTX_FAIL("rtx_srf_pixel_cube_fit: flags=%u, only RTX_FIT_START_GIVEN is defined", flags);
  ScfArgs a;
  if (scf_front("rtx_srf_pixel_cube_fit", a, nB, Q, T_node_h, nEnd, nPix, nMix)) return 1;
  if (max_iter < 0 || max_iter > SCF_ITER_MAX) RTX_FAIL("rtx_srf_pixel_cube_fit: max_iter=%d outside [0,%d]", max_iter, SCF_ITER_MAX);
  if (!isfinite(lambda0) || lambda0 < 0.0) RTX_FAIL("rtx_srf_pixel_cube_fit: lambda0=%g: finite and not negative", lambda0);
  if (!isfinite(ftol) || ftol < 0.0) RTX_FAIL("rtx_srf_pixel_cube_fit: ftol=%g: finite and not negative", ftol);
  if (!meas || !frac || !Tpix || !cost || !n_iter || !status)
    RTX_FAIL("rtx_srf_pixel_cube_fit: a required pointer is NULL (meas, frac, Tpix, cost, n_iter, status)");
  if (nB == 0 || nPix == 0) return 0;
  if (!N || !C || !tab || !kidx) RTX_FAIL("rtx_srf_pixel_cube_fit: a required pointer is NULL");
  a.N = N; a.C = C; a.tab = tab; a.kidx = kidx; a.meas = meas; a.wgt = wgt;
  a.frac = frac; a.Tpix = Tpix; a.max_iter = max_iter; a.given = (flags & RTX_FIT_START_GIVEN) ? 1 : 0;
  a.lambda0 = lambda0; a.ftol = ftol;
  a.cost = cost; a.n_iter = n_iter; a.status = status; a.hess = hess;
  scf_launch(a, Q, nMix, true, (hipStream_t)stream);
  RTX_LAUNCH_CHECK();
  return 0;
}
