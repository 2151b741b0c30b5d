// The bound-constrained per-pixel fit to a measured HSI cube (include/radtxfr_hip.h, rtx_srf_pixel_cube_normal_box and
// rtx_srf_pixel_cube_fit_box): rtx_srf_cube_fit.hip's problem in the box T_lo <= T <= T_hi, f_m >= 0, with an
// optional soft sum-to-one. Lane = pixel, one wave per workgroup, templates on <Q, nMix>; the evaluation is scf_eval itself
// (rtx_srf_cube_fit_common.h), so cost, grad and H of the real bands have the unconstrained kernels' bits.
//
// The pseudo-band (scfb_pseudo), after the band loop, when sum_weight = delta > 0:
//   r_s = (sum_m (double)f_m, m ascending, plain adds) - 1;  cost = fma(delta r_s, r_s, cost);
//   grad_m = fma(1, delta r_s, grad_m);  H_mm' = fma(delta, 1, H_mm'), m, m' >= 1.
// The box step (scfb_step) from u = (T, (double)f_m) with lo = (T_lo, 0, ..), hi = (T_hi, +inf, ..):
//   1 B = { i : (u_i <= lo_i and g_i > 0) or (u_i >= hi_i and g_i < 0) } (and whatever the caller holds), s_i = 0 on it;
//   2 a pass (scfb_solve): scf_solve's Cholesky on the matrix whose rows and columns of B are the identity's (A_ii = 1, not
//     damped) and whose right-hand side is s_i on B and -(g_j + sum_{i in B} H_ji s_i), i ascending by fma, off it: selects
//     on a per-lane bit mask, H is never indexed dynamically; an L entry of a row or column of B is an exact 0, so the free
//     block has the bits of its own Cholesky. d_i = s_i on B. Every free i with u_i + d_i < lo_i (> hi_i) joins B with
//     s_i = lo_i - u_i (hi_i - u_i). At most 1 + nMix passes; the loop ends when no lane of the wave joined (a lane that is
//     done solves the same system again: the same bits). What joins in pass 1 + nMix was the last free unknown: d_i = s_i.
//   3 the trial (scfb_trial): T' = clamp(T + d_0), f'_m = max(0f, (float)((double)f_m + d_m)), max(0f, x) = x > 0 ? x : 0.
// The fit is scf_fit_kernel's loop with one call of scf_eval in it; the node scan's second evaluation is at the box solve of
// the fraction block (T held in B, lambda 0, from f = 0), and a trial point that equals the current point bit for bit stops
// the lane with status 0 before it is evaluated.
#include "rtx_srf_cube_fit_common.h"  // SCF_PB, SCF_TAB_LDS: rtx_srf_cube_fit.hip's values

#define SCFB_MIX_MAX 4  // rtx_srf_pixel_cube_fit_box_max_mix(): every instantiation without scratch (profiles/cube_fit_box_resources.txt)

struct ScfBoxArgs : ScfArgs {
  double sum_weight;
  int* active;  // [nPix] or NULL
};

// Keeps a value in vector registers from here on. The fit kernel forms its per-lane output addresses and the few uniform
// arguments that only the step and the stops read this way before the loop: held as scalars through the whole loop they
// do not fit beside scf_eval's (the scalar file is full, profiles/cube_fit_box_resources.txt). This and the bitwise
// selects below are hints to the register allocator, not guarantees: a new compiler can bring the spills back without any
// error, so re-run `make resources` and compare with that record whenever ROCm is updated.
template <class V>
__device__ __forceinline__ V scfb_vec(V x) {
  asm volatile("" : "+v"(x));
  return x;
}

template <int NM>
__device__ __forceinline__ void scfb_pseudo(double delta, const float (&f)[NM], ScfSums<NM>& o) {
  if (!(delta > 0.0)) return;  // the same for every lane
  double sum = (double)f[0];
#pragma unroll
  for (int m = 1; m < NM; ++m) sum = sum + (double)f[m];
  const double r = sum - 1.0, dr = delta * r;
  o.c = fma(dr, r, o.c);
#pragma unroll
  for (int i = 1; i <= NM; ++i) {
    o.g[i] = fma(1.0, dr, o.g[i]);
#pragma unroll
    for (int j = 1; j <= i; ++j) o.H[scf_tri(i, j)] = fma(delta, 1.0, o.H[scf_tri(i, j)]);
  }
}

// m ? x : y for a mask m of all ones or all zeros held in a vector register: bitwise, so that the 1 + nMix masks of a pass
// and their pairs do not each take a pair of scalar registers the way compare results do.
__device__ __forceinline__ double scfb_sel(unsigned m, double x, double y) {
  const unsigned long long mm = ((unsigned long long)m << 32) | m;
  return __longlong_as_double((long long)(((unsigned long long)__double_as_longlong(x) & mm) | ((unsigned long long)__double_as_longlong(y) & ~mm)));
}

// One pass: the unknowns of the bit mask B take d_i = sv_i, the others the damped Cholesky step of their own block. The
// selects build the matrix and the right-hand side first; the factor then overwrites the matrix in place, as scf_solve
// computes it.
template <int NM>
__device__ __forceinline__ bool scfb_solve(const ScfSums<NM>& s, double lam, unsigned B, const double (&sv)[NM + 1], double (&d)[NM + 1]) {
  constexpr int N = NM + 1;
  double L[N * (N + 1) / 2], z[N];
  unsigned m[N];
#pragma unroll
  for (int i = 0; i < N; ++i) m[i] = scfb_vec(0u - ((B >> i) & 1u));
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double r = s.g[i];
#pragma unroll
    for (int kk = 0; kk < N; ++kk) {
      if (kk == i) continue;
      const double h = kk < i ? s.H[scf_tri(i, kk)] : s.H[scf_tri(kk, i)];
      r = scfb_sel(m[kk], fma(h, sv[kk], r), r);
    }
    z[i] = scfb_sel(m[i], sv[i], -r);
#pragma unroll
    for (int j = 0; j < i; ++j) L[scf_tri(i, j)] = scfb_sel(m[i] | m[j], 0.0, s.H[scf_tri(i, j)]);
    const double hii = scfb_sel(m[i], 1.0, s.H[scf_tri(i, i)]);
    L[scf_tri(i, i)] = fma(scfb_sel(m[i], 0.0, lam), hii, hii);
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double piv = L[scf_tri(j, j)];
#pragma unroll
    for (int kk = 0; kk < j; ++kk) piv = fma(-L[scf_tri(j, kk)], L[scf_tri(j, kk)], piv);
    ok = ok && piv > 0.0 && piv <= 1.79769313486231570815e308;  // false for NaN and infinity
    const double ljj = sqrt(piv);
    L[scf_tri(j, j)] = ljj;
#pragma unroll
    for (int i = j + 1; i < N; ++i) {
      double v = L[scf_tri(i, j)];
#pragma unroll
      for (int kk = 0; kk < j; ++kk) v = fma(-L[scf_tri(i, kk)], L[scf_tri(j, kk)], v);
      L[scf_tri(i, j)] = v / ljj;
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double v = z[i];
#pragma unroll
    for (int kk = 0; kk < i; ++kk) v = fma(-L[scf_tri(i, kk)], z[kk], v);
    z[i] = v / L[scf_tri(i, i)];
  }
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    double v = z[i];
#pragma unroll
    for (int kk = N - 1; kk > i; --kk) v = fma(-L[scf_tri(kk, i)], d[kk], v);
    d[i] = v / L[scf_tri(i, i)];
  }
#pragma unroll
  for (int i = 0; i < N; ++i) d[i] = ok ? scfb_sel(m[i], sv[i], d[i]) : __builtin_nan("");
  return ok;
}

// The box step from u = (T, f) on the sums s. hold: unknowns the caller keeps in B with s_i = 0. B: the set at the end.
// False: a pass met a pivot that was not finite or not positive, d is NaN. The pass loop's exit is uniform over the lanes
// that are in it together.
template <int NM>
__device__ __forceinline__ bool scfb_step(const ScfSums<NM>& s, double lam, double T, const float (&f)[NM], double T_lo, double T_hi,
                                          unsigned hold, double (&d)[NM + 1], unsigned& B) {
  constexpr int NU = NM + 1;
  double u[NU], sv[NU];
  u[0] = T;
#pragma unroll
  for (int m = 0; m < NM; ++m) u[m + 1] = (double)f[m];
  B = hold;
  if ((T <= T_lo && s.g[0] > 0.0) || (T >= T_hi && s.g[0] < 0.0)) B |= 1u;
  sv[0] = 0.0;
#pragma unroll
  for (int i = 1; i < NU; ++i) {
    if (u[i] <= 0.0 && s.g[i] > 0.0) B |= 1u << i;  // hi_i = +inf: no finite fraction is on it
    sv[i] = 0.0;
  }
  bool ok = true;
#pragma unroll 1
  for (int pass = 0; pass < NU; ++pass) {
    ok = scfb_solve<NM>(s, lam, B, sv, d);
    unsigned joined = 0;
    {
      const double x = u[0] + d[0];
      const bool free = !(B & 1u), jl = free && x < T_lo, jh = free && x > T_hi;
      sv[0] = jl ? T_lo - u[0] : (jh ? T_hi - u[0] : sv[0]);
      joined |= (jl || jh) ? 1u : 0u;
    }
#pragma unroll
    for (int i = 1; i < NU; ++i) {
      const bool jl = !((B >> i) & 1u) && u[i] + d[i] < 0.0;
      sv[i] = jl ? 0.0 - u[i] : sv[i];
      joined |= jl ? 1u << i : 0u;
    }
    B |= joined;
    if (!__any(joined != 0u)) break;
  }
#pragma unroll
  for (int i = 0; i < NU; ++i) d[i] = ok ? (((B >> i) & 1u) ? sv[i] : d[i]) : d[i];  // what joined in the last pass
  return ok;
}

template <int NM>
__device__ __forceinline__ void scfb_trial(double T_lo, double T_hi, double T, const float (&f)[NM], const double (&d)[NM + 1],
                                           double& Tt, float (&ft)[NM]) {
  double x = T + d[0];
  x = x < T_lo ? T_lo : x;
  Tt = x > T_hi ? T_hi : x;
#pragma unroll
  for (int m = 0; m < NM; ++m) {
    const float v = (float)((double)f[m] + d[m + 1]);
    ft[m] = v > 0.f ? v : 0.f;
  }
}

// Step 1's set alone: the unknowns on a bound whose gradient points out of the box.
template <int NM>
__device__ __forceinline__ unsigned scfb_kkt(double T_lo, double T_hi, const ScfSums<NM>& s, double T, const float (&f)[NM]) {
  unsigned B = 0;
  if ((T <= T_lo && s.g[0] > 0.0) || (T >= T_hi && s.g[0] < 0.0)) B |= 1u;
#pragma unroll
  for (int m = 0; m < NM; ++m)
    if ((double)f[m] <= 0.0 && s.g[m + 1] > 0.0) B |= 1u << (m + 1);
  return B;
}

template <int Q, int NM>
__global__ __launch_bounds__(SCF_PB) void scfb_normal_kernel(ScfBoxArgs a) {
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
    k[m] = min(max(a.kidx[p * NM + m], 0), a.nEnd - 1);
  }
  ScfSums<NM> o;
  scf_eval<Q, NM>(a, reinterpret_cast<float*>(s_dyn), p, T, f, k, o);
  scfb_pseudo<NM>(a.sum_weight, f, o);
  double d[NU];
  unsigned B = 0;
  if (a.step || a.active) scfb_step<NM>(o, a.lambda ? a.lambda[p] : 0.0, T, f, a.T_lo, a.T_hi, 0u, d, B);  // uniform: every lane is in it
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
#pragma unroll
    for (int i = 0; i < NU; ++i) a.step[p * NU + i] = ok ? d[i] : nan;
  }
  if (a.active) a.active[p] = ok ? (int)B : 0;
}

template <int Q, int NM>
__global__ __launch_bounds__(SCF_PB) void scfb_fit_kernel(ScfBoxArgs a) {
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
      const float v = a.frac[p * NM + m];
      fin = fin && fabsf(v) <= 3.40282346638528859812e38f;  // false for NaN and infinity
      f[m] = ft[m] = v > 0.f ? v : 0.f;                      // the start projected into the box
    }
    if (!fin && status < 0) status = 2;
    if (!fin) {  // a stand-in: the lane rides along, nothing of it is kept
      T = Tt = a.T_lo;
#pragma unroll
      for (int m = 0; m < NM; ++m) f[m] = ft[m] = 0.f;
    }
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
  // the lane's own output addresses (a NULL optional output stays NULL) and the step's and the stops' arguments
  double* const o_T = scfb_vec(a.Tpix + p);
  float* const o_f = scfb_vec(a.frac + p * NM);
  double* const o_cost = scfb_vec(a.cost + p);
  int* const o_iter = scfb_vec(a.n_iter + p);
  int* const o_status = scfb_vec(a.status + p);
  double* const o_hess = scfb_vec(a.hess ? a.hess + p * NH : nullptr);
  double* const o_grad = scfb_vec(a.grad ? a.grad + p * NU : nullptr);
  int* const o_active = scfb_vec(a.active ? a.active + p : nullptr);
  const double T_lo = scfb_vec(a.T_lo), T_hi = scfb_vec(a.T_hi), ftol = scfb_vec(a.ftol);
  const int max_iter = scfb_vec(a.max_iter);
  const double delta = scfb_vec(a.sum_weight);
  const int mine = scfb_vec(p_own < a.nPix ? 1 : 0);
  for (int e = 0;; ++e) {
    const bool pre = e < n_pre;
    if (pre) {
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
    } else {
      bool want = false;  // a trial step is wanted
      if (status < 0) {
        if (cur.c == 0.0) status = 0;
        else if (n_iter >= max_iter) status = 1;
        else want = true;
      }
      if (__any(want)) {  // every lane solves (a stopped lane's step is dropped): the pass loop's exit stays uniform
        double d[NU];
        unsigned B;
        const bool ok = scfb_step<NM>(cur, lam, T, f, T_lo, T_hi, 0u, d, B);
        double Tn_;
        float fn_[NM];
        scfb_trial<NM>(T_lo, T_hi, T, f, d, Tn_, fn_);
        bool moved = Tn_ != T;
#pragma unroll
        for (int m = 0; m < NM; ++m) moved = moved || fn_[m] != f[m];
        // singular: 3. The trial point is the current point: 0, not evaluated, not counted.
        status = want ? (!ok ? 3 : (!moved ? 0 : status)) : status;
        const bool go = want && ok;
        Tt = go ? Tn_ : Tt;
#pragma unroll
        for (int m = 0; m < NM; ++m) ft[m] = go ? fn_[m] : ft[m];
      }
    }
    if (!__syncthreads_or(pre || status < 0)) break;
    scf_eval<Q, NM>(a, reinterpret_cast<float*>(s_dyn), p, Tt, ft, k, tr);
    scfb_pseudo<NM>(delta, ft, tr);
    if (pre) {
      if (given) {
        cur = tr;
      } else if (!(e & 1)) {  // the box solve of the fraction block, undamped, from the evaluation at f = 0: T is held
        double d[NU];
        unsigned B;
        node_ok = scfb_step<NM>(tr, 0.0, Tt, ft, T_lo, T_hi, 1u, d, B);
        const double Tq = Tt;
        if (node_ok) scfb_trial<NM>(T_lo, T_hi, Tq, ft, d, Tt, ft);  // d_0 is 0: Tt stays the node
        Tt = Tq;
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
        if (was - cur.c < ftol * was) status = 0;
      } else {
        lam = fmin(10.0 * lam, SCF_LAM_MAX);
        if (lam >= SCF_LAM_MAX) status = 0;
      }
    }
  }
  if (!mine) return;
  const bool good = status < 2;
  const double nan = __builtin_nan("");
  *o_T = good ? T : nan;
#pragma unroll
  for (int m = 0; m < NM; ++m) o_f[m] = good ? f[m] : __builtin_nanf("");
  *o_cost = good ? cur.c : nan;
  *o_iter = n_iter;
  *o_status = status;
  if (o_hess) {
#pragma unroll
    for (int i = 0; i < NH; ++i) o_hess[i] = good ? cur.H[i] : nan;
  }
  if (o_grad) {
#pragma unroll
    for (int i = 0; i < NU; ++i) o_grad[i] = good ? cur.g[i] : nan;
  }
  if (o_active) *o_active = good ? (int)scfb_kkt<NM>(T_lo, T_hi, cur, T, f) : 0;
}

template <int Q, int NM>
static void launch_scfb(const ScfBoxArgs& a, bool fit, hipStream_t st) {
  const dim3 grid((unsigned)((a.nPix + SCF_PB - 1) / SCF_PB));
  const size_t lds = (size_t)a.stride * 64 * sizeof(float);
  if (fit) hipLaunchKernelGGL((scfb_fit_kernel<Q, NM>), grid, dim3(SCF_PB), lds, st, a);
  else hipLaunchKernelGGL((scfb_normal_kernel<Q, NM>), grid, dim3(SCF_PB), lds, st, a);
}

template <int Q>
static void launch_scfb_mix(const ScfBoxArgs& a, int nMix, bool fit, hipStream_t st) {
  switch (nMix) {
    case 1: launch_scfb<Q, 1>(a, fit, st); break;
    case 2: launch_scfb<Q, 2>(a, fit, st); break;
    case 3: launch_scfb<Q, 3>(a, fit, st); break;
    default: launch_scfb<Q, 4>(a, fit, st); break;
  }
}

static void scfb_launch(const ScfBoxArgs& a, int Q, int nMix, bool fit, hipStream_t st) {
  switch (Q) {
    case 1: launch_scfb_mix<1>(a, nMix, fit, st); break;
    case 2: launch_scfb_mix<2>(a, nMix, fit, st); break;
    case 3: launch_scfb_mix<3>(a, nMix, fit, st); break;
    case 4: launch_scfb_mix<4>(a, nMix, fit, st); break;
    case 5: launch_scfb_mix<5>(a, nMix, fit, st); break;
    case 6: launch_scfb_mix<6>(a, nMix, fit, st); break;
    case 7: launch_scfb_mix<7>(a, nMix, fit, st); break;
    default: launch_scfb_mix<8>(a, nMix, fit, st); break;
  }
}

// scf_front, then what the box entries add to it.
static int scfb_front(const char* fn, ScfBoxArgs& a, int nB, int Q, const double* T_node_h, int nEnd, int64_t nPix, int nMix, double sum_weight) {
  if (scf_front(fn, a, nB, Q, T_node_h, nEnd, nPix, nMix)) return 1;
  a.sum_weight = 0.0;
  a.active = nullptr;
  if (nMix > SCFB_MIX_MAX) RTX_FAIL("%s: nMix=%d above rtx_srf_pixel_cube_fit_box_max_mix() = %d", fn, nMix, SCFB_MIX_MAX);
  if (!isfinite(sum_weight) || sum_weight < 0.0) RTX_FAIL("%s: sum_weight=%g: finite and not negative", fn, sum_weight);
  a.sum_weight = sum_weight;
  return 0;
}

extern "C" int rtx_srf_pixel_cube_fit_box_max_mix(void) { return SCFB_MIX_MAX; }

extern "C" int rtx_srf_pixel_cube_normal_box(int nB, int Q, const double* T_node_h, const float* N, const float* C, const float* tab, int nEnd,
                                             int64_t nPix, int nMix, const int32_t* kidx, const float* frac, const double* Tpix,
                                             const float* meas, const float* wgt, const double* lambda, double* cost, double* grad, double* hess,
                                             double* step, void* stream, unsigned flags, double sum_weight, int32_t* active) {
  if (flags != 0) RTX_FAIL("rtx_srf_pixel_cube_normal_box: flags=%u, none is defined", flags);
  ScfBoxArgs a;
  if (scfb_front("rtx_srf_pixel_cube_normal_box", a, nB, Q, T_node_h, nEnd, nPix, nMix, sum_weight)) return 1;
  if (!meas || !cost) RTX_FAIL("rtx_srf_pixel_cube_normal_box: a required pointer is NULL (meas, cost)");
  if (nB == 0 || nPix == 0) return 0;
  if (!N || !C || !tab || !kidx || !frac || !Tpix) RTX_FAIL("rtx_srf_pixel_cube_normal_box: a required pointer is NULL");
  a.N = N; a.C = C; a.tab = tab; a.kidx = kidx; a.meas = meas; a.wgt = wgt;
  a.frac_in = frac; a.T_in = Tpix; a.lambda = lambda;
  a.cost = cost; a.grad = grad; a.hess = hess; a.step = step; a.active = active;
  scfb_launch(a, Q, nMix, false, (hipStream_t)stream);
  RTX_LAUNCH_CHECK();
  return 0;
}

extern "C" int rtx_srf_pixel_cube_fit_box(int nB, int Q, const double* T_node_h, const float* N, const float* C, const float* tab, int nEnd,
                                          int64_t nPix, int nMix, const int32_t* kidx, const float* meas, const float* wgt, float* frac,
                                          double* Tpix, int max_iter, double lambda0, double ftol, double* cost, int32_t* n_iter,
                                          int32_t* status, double* hess, void* stream, unsigned flags, double sum_weight, double* grad,
                                          int32_t* active) {
  if (flags & ~(unsigned)RTX_FIT_START_GIVEN) RTX_FAIL("rtx_srf_pixel_cube_fit_box: flags=%u, only RTX_FIT_START_GIVEN is defined", flags);
  ScfBoxArgs a;
  if (scfb_front("rtx_srf_pixel_cube_fit_box", a, nB, Q, T_node_h, nEnd, nPix, nMix, sum_weight)) return 1;
  if (max_iter < 0 || max_iter > SCF_ITER_MAX) RTX_FAIL("rtx_srf_pixel_cube_fit_box: max_iter=%d outside [0,%d]", max_iter, SCF_ITER_MAX);
  if (!isfinite(lambda0) || lambda0 < 0.0) RTX_FAIL("rtx_srf_pixel_cube_fit_box: lambda0=%g: finite and not negative", lambda0);
  if (!isfinite(ftol) || ftol < 0.0) RTX_FAIL("rtx_srf_pixel_cube_fit_box: ftol=%g: finite and not negative", ftol);
  if (!meas || !frac || !Tpix || !cost || !n_iter || !status)
    RTX_FAIL("rtx_srf_pixel_cube_fit_box: a required pointer is NULL (meas, frac, Tpix, cost, n_iter, status)");
  if (nB == 0 || nPix == 0) return 0;
  if (!N || !C || !tab || !kidx) RTX_FAIL("rtx_srf_pixel_cube_fit_box: a required pointer is NULL");
  a.N = N; a.C = C; a.tab = tab; a.kidx = kidx; a.meas = meas; a.wgt = wgt;
  a.frac = frac; a.Tpix = Tpix; a.max_iter = max_iter; a.given = (flags & RTX_FIT_START_GIVEN) ? 1 : 0;
  a.lambda0 = lambda0; a.ftol = ftol;
  a.cost = cost; a.n_iter = n_iter; a.status = status; a.hess = hess; a.grad = grad; a.active = active;
  scfb_launch(a, Q, nMix, true, (hipStream_t)stream);
  RTX_LAUNCH_CHECK();
  return 0;
}
