// Tangent-linear TUD: out[vec][row][nu] = sum_w sum_l J[w][l][row][nu] v[vec][w][l] with J what
// rtx_tud_jacobian defines, for tangent vectors v on (layer T, mixing ratios). J is never stored and never formed
// per layer: the tangents are carried through the recurrences of rtx_tud, one pass each, O(nL) per point for tau and
// L-up and O(nL N_angle) for Ld.
//
// rtx_tud_jvp : per point and vector, dOD_l = (dOD/dT)_l v_T[l] + sum_s K_s,l v_s[l], with (dOD/dT)_l the float32 number
//               tud_jac_kernel forms. Then
//                 tau rows : -mu tau sum_{mask} dOD_l                      (return_od: mu sum_{mask} dOD_l)
//                 L-up     : dL^l = t_l dL^(l-1) + mu t_l D_l dOD_l + (1 - t_l) (dB/dT)_l v_T[l],  D_l = B_l - L^(l-1),
//                            written for each altitude when the sweep reaches its count
//                 Ld       : per stream q, top-down from n_down - 1,
//                            dR_l = t_l,q dR_(l+1) + (1/c_q) t_l,q E_l,q dOD_l + (1 - t_l,q) (dB/dT)_l v_T[l],
//                            E_l,q = B_l - R_(l+1),q;  dLd = sum_q omega_q dR_0,q
//               D and E are the float32 recurrences of tud_jac_kernel (fp64 differences of neighbouring layers' B), the
//               transmittances, emissivities, B and dB/dT its device functions; every product with a tangent and every
//               sum of tangents is fp64, and the result is rounded to float32 once, at the store.
//
// Mapping (CDNA4): lane <-> wavenumber, 256-thread workgroups, as the sibling kernels. No cross-lane operation, no LDS,
// no atomics: a point's value is a function of its column and of the vectors alone, whatever the shard or the launch.
// The vectors of a launch (at most TUDT_NV) share the column reads, D, E and every transcendental; V is read through
// wave-uniform addresses (scalar loads). A row group that is not requested is compiled out (template flags): no Ld ->
// no stream sweeps; no L-up and no Ld -> no Planck work; no tau -> tau is not read.
#include "rtx_tud_jac_common.h"

#define TUDT_NV 4  // tangent vectors per launch: [TUDT_NV][TUDJ_QG] fp64 stream tangents stay in registers, no scratch

struct TudJvpArgs {
  TudJacArgs c;     // the column (J, lay and n_lay unused)
  const double* V;  // [nv][n_wrt][n_layers], wrt slots as J's (T at t_pos); library-owned staging
  float* d_tau;     // [nv][n_alt][ld_out] or NULL
  float* d_Lu;      // [nv][n_alt][ld_out] or NULL
  float* d_Ld;      // [nv][ld_out] or NULL
  long long ld_out;
  int nv;
  unsigned prefix;  // bit a: the tau mask of altitude a is its first count[a] layers (always, for sorted Z)
};
static_assert(sizeof(TudJvpArgs) <= 4096, "kernel arguments are limited to 4 KiB");

// dOD_l of every vector and the vectors' v_T[l], fp64: T first, then the species in K's order
__device__ __forceinline__ void tangent_od(const TudJvpArgs& v, long long i, int j, int n_wrt, double (&dod)[TUDT_NV],
                                           double (&vt)[TUDT_NV]) {
  const TudJacArgs& a = v.c;
  const int nL = a.n_layers;
  const size_t e = (size_t)j * a.ld + i;
#pragma unroll
  for (int vv = 0; vv < TUDT_NV; ++vv) dod[vv] = vt[vv] = 0.0;
  if (a.with_T) {
    const double d = (double)((a.ODp[e] - a.ODm[e]) * a.inv_2h);
#pragma unroll
    for (int vv = 0; vv < TUDT_NV; ++vv)
      if (vv < v.nv) {
        vt[vv] = v.V[((size_t)vv * n_wrt + a.t_pos) * nL + j];
        dod[vv] = d * vt[vv];
      }
  }
  for (int s = 0; s < a.n_spec; ++s) {
    const int slot = a.with_T && s >= a.t_pos ? s + 1 : s;
    const double d = (double)a.K[(size_t)s * nL * a.ld + e];
#pragma unroll
    for (int vv = 0; vv < TUDT_NV; ++vv)
      if (vv < v.nv) dod[vv] = fma(d, v.V[((size_t)vv * n_wrt + slot) * nL + j], dod[vv]);
  }
}

template <bool TAU, bool LU, bool LD>
__global__ __launch_bounds__(256) void tud_jvp_kernel(TudJvpArgs v) {
  const TudJacArgs& a = v.c;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.g.n) return;  // no cross-lane work: dead lanes leave
  const int nL = a.n_layers;
  const float* __restrict__ od = a.OD + i;
  const int n_wrt = a.with_T + a.n_spec;
  const size_t vstride = (size_t)a.n_alt * v.ld_out;  // one vector of d_tau / d_Lu
  double x = 0.0, c1x3 = 0.0;
  if constexpr (LU || LD) {
    x = grid_x(a.g, a.g.offset + i);
    const double x100 = x * 100.0;
    c1x3 = RT_C1 * (x100 * x100 * x100) * 1e4;
  }
  double dod[TUDT_NV], vt[TUDT_NV];

  // ---- bottom-up: the prefix sums of dOD (tau rows) and the L-up tangent, each altitude written at its count ----
  if constexpr (TAU || LU) {
    int cmax = 0;
    for (int q = 0; q < a.n_alt; ++q) cmax = max(cmax, a.count[q]);
    const int jend = TAU ? nL : cmax;  // L-up alone stops at the highest count
    double P[TUDT_NV], dL[TUDT_NV];
#pragma unroll
    for (int vv = 0; vv < TUDT_NV; ++vv) P[vv] = dL[vv] = 0.0;
    double Bc = 0.0;
    float D = 0.f;
    if constexpr (LU) {
      Bc = planck_f64(c1x3, x, a.c2l2e_over_T[0]);
      D = (float)Bc;
    }
    for (int j = 0; j <= jend; ++j) {
      for (int q = 0; q < a.n_alt; ++q) {
        if (a.count[q] != j) continue;  // wave-uniform
        if constexpr (LU) {
#pragma unroll
          for (int vv = 0; vv < TUDT_NV; ++vv)
            if (vv < v.nv) v.d_Lu[vv * vstride + (size_t)q * v.ld_out + i] = (float)dL[vv];
        }
        if constexpr (TAU) {
          if ((v.prefix >> q) & 1u) {
            const float gT = a.return_od ? a.mu : -a.mu * a.tau[(size_t)q * a.ld_tau + i];
#pragma unroll
            for (int vv = 0; vv < TUDT_NV; ++vv)
              if (vv < v.nv) v.d_tau[vv * vstride + (size_t)q * v.ld_out + i] = (float)((double)gT * P[vv]);
          }
        }
      }
      if (j == jend) break;
      const float o = od[(size_t)j * a.ld];
      tangent_od(v, i, j, n_wrt, dod, vt);
      if constexpr (TAU) {
#pragma unroll
        for (int vv = 0; vv < TUDT_NV; ++vv) P[vv] += dod[vv];
      }
      if constexpr (LU) {
        if (j < cmax) {
          const float t = __builtin_amdgcn_exp2f(-(o * a.mu) * (float)LOG2E);
          const double gU = (double)(a.mu * t) * (double)D;  // mu t_l D_l
          double hU = 0.0;                                   // (1 - t_l) dB_l
          if (a.with_T) {
            float B, dB;
            planck_dT(c1x3, x, a.c2l2e_over_T[j], B, dB);
            hU = (double)one_minus_exp_neg(o * a.mu) * (double)dB;
          }
#pragma unroll
          for (int vv = 0; vv < TUDT_NV; ++vv)
            if (vv < v.nv) dL[vv] = fma((double)t, dL[vv], fma(gU, dod[vv], hU * vt[vv]));
          if (j + 1 < cmax) {  // D_{j+1}, as tud_jac_kernel carries it
            const double Bn = planck_f64(c1x3, x, a.c2l2e_over_T[j + 1]);
            D = fmaf(t, D, (float)(Bn - Bc));
            Bc = Bn;
          }
        }
      }
    }
    // a tau mask that is not a run of the lowest layers (unsorted Z): a sweep of its own
    if constexpr (TAU) {
      for (int q = 0; q < a.n_alt; ++q) {
        if ((v.prefix >> q) & 1u) continue;
#pragma unroll
        for (int vv = 0; vv < TUDT_NV; ++vv) P[vv] = 0.0;
        for (int j = 0; j < nL; ++j) {
          if (!((a.lbits[j] >> q) & 1u)) continue;
          tangent_od(v, i, j, n_wrt, dod, vt);
#pragma unroll
          for (int vv = 0; vv < TUDT_NV; ++vv) P[vv] += dod[vv];
        }
        const float gT = a.return_od ? a.mu : -a.mu * a.tau[(size_t)q * a.ld_tau + i];
#pragma unroll
        for (int vv = 0; vv < TUDT_NV; ++vv)
          if (vv < v.nv) v.d_tau[vv * vstride + (size_t)q * v.ld_out + i] = (float)((double)gT * P[vv]);
      }
    }
  }

  // ---- downwelling: the stream tangents top-down, TUDJ_QG streams at a time ----
  if constexpr (LD) {
    double acc[TUDT_NV];
#pragma unroll
    for (int vv = 0; vv < TUDT_NV; ++vv) acc[vv] = 0.0;
    if (a.n_down > 0) {
      for (int q0 = 0; q0 < a.n_str; q0 += TUDJ_QG) {
        double Bt = planck_f64(c1x3, x, a.c2l2e_over_T[a.n_down - 1]);
        float E[TUDJ_QG];
        double dR[TUDT_NV][TUDJ_QG];
#pragma unroll
        for (int q = 0; q < TUDJ_QG; ++q) {
          E[q] = (float)Bt;
#pragma unroll
          for (int vv = 0; vv < TUDT_NV; ++vv) dR[vv][q] = 0.0;
        }
        for (int j = a.n_down - 1; j >= 0; --j) {
          const float o = od[(size_t)j * a.ld];
          tangent_od(v, i, j, n_wrt, dod, vt);
          float dB = 0.f;
          if (a.with_T) {
            float B;
            planck_dT(c1x3, x, a.c2l2e_over_T[j], B, dB);
          }
          double dBn = 0.0;
          if (j > 0) {
            const double Bn = planck_f64(c1x3, x, a.c2l2e_over_T[j - 1]);
            dBn = Bn - Bt;
            Bt = Bn;
          }
#pragma unroll
          for (int q = 0; q < TUDJ_QG; ++q) {
            if (q0 + q < a.n_str) {
              const double ic = a.str_ic[q0 + q];
              const float y = o * (float)ic;
              const float t = __builtin_amdgcn_exp2f(-y * (float)LOG2E);
              const double gR = ic * (double)t * (double)E[q];           // (1/c_q) t_l,q E_l,q
              const double hR = (double)one_minus_exp_neg(y) * (double)dB;  // (1 - t_l,q) dB_l
#pragma unroll
              for (int vv = 0; vv < TUDT_NV; ++vv)
                if (vv < v.nv) dR[vv][q] = fma((double)t, dR[vv][q], fma(gR, dod[vv], hR * vt[vv]));
              E[q] = fmaf(t, E[q], (float)dBn);  // E_{j-1}, as tud_jac_kernel carries it (unused after j = 0)
            }
          }
        }
#pragma unroll
        for (int q = 0; q < TUDJ_QG; ++q)
          if (q0 + q < a.n_str) {
#pragma unroll
            for (int vv = 0; vv < TUDT_NV; ++vv) acc[vv] = fma((double)a.str_w[q0 + q], dR[vv][q], acc[vv]);
          }
      }
    }
    // N_angle = 1: no stream has weight, compute_TUD's Ld is 0/0 (NaN), and so is its tangent
#pragma unroll
    for (int vv = 0; vv < TUDT_NV; ++vv)
      if (vv < v.nv) v.d_Ld[(size_t)vv * v.ld_out + i] = a.n_str == 0 ? NAN : (float)acc[vv];
  }
}

// V on the device, per (device, stream): calls on one stream are ordered by it
static StreamScratch* const jvp_stage = new StreamScratch();

extern "C" int rtx_tud_jvp_max_vectors(void) { return TUDT_NV; }

static int tud_jvp_run(const TudColumnIn& c, const double* V_h, int n_vec, float* d_tau, float* d_Lu, float* d_Ld, int64_t ld_out,
                       void* stream) {
  if (tud_column_check(c)) return 1;
  if (!d_tau && !d_Lu && !d_Ld) RTX_FAIL("no output: d_tau, d_Lu and d_Ld are all NULL");
  if (n_vec < 1 || n_vec > TUDT_NV) RTX_FAIL("n_vec=%d outside [1,%d] (rtx_tud_jvp_max_vectors)", n_vec, TUDT_NV);
  if (!V_h) RTX_FAIL("V_h is NULL");
  TudJvpArgs v;
  const int32_t layer0 = 0;  // the request's layer list is not this entry point's: every layer takes part through V
  if (tud_jac_setup(v.c, c, d_tau != nullptr, &layer0, 1)) return 1;
  if (ld_out < c.grid->n) RTX_FAIL("ld_out=%lld smaller than the shard", (long long)ld_out);
  const size_t cnt = (size_t)n_vec * (size_t)(v.c.with_T + c.n_spec) * (size_t)c.n_layers;
  for (size_t t = 0; t < cnt; ++t)
    if (!isfinite(V_h[t])) RTX_FAIL("V_h[%zu] is not finite", t);
  if (c.grid->n == 0) return 0;
  unsigned blocks;
  if (tud_blocks(c.grid, 256, &blocks)) return 1;
  v.prefix = 0;
  for (int ia = 0; ia < c.n_alt; ++ia) {
    bool run = true;
    for (int k = 0; k < v.c.count[ia]; ++k) run = run && ((v.c.lbits[k] >> ia) & 1u);
    if (run) v.prefix |= 1u << ia;
  }
  hipStream_t st = (hipStream_t)stream;
  void* V_d = nullptr;
  if (jvp_stage->get(st, cnt * sizeof(double), &V_d)) return 1;
  RTX_HIP(hipMemcpyAsync(V_d, V_h, cnt * sizeof(double), hipMemcpyHostToDevice, st));  // pageable: staged before returning
  v.V = (const double*)V_d; v.d_tau = d_tau; v.d_Lu = d_Lu; v.d_Ld = d_Ld; v.ld_out = ld_out; v.nv = n_vec;
  tud_dispatch_rows(d_tau, d_Lu, d_Ld, [&](auto tau, auto up, auto down) {
    hipLaunchKernelGGL((tud_jvp_kernel<decltype(tau)::value, decltype(up)::value, decltype(down)::value>), dim3(blocks), dim3(256),
                       0, st, v);
  });
  RTX_LAUNCH_CHECK();
  return 0;
}

extern "C" int rtx_tud_jvp(const float* OD, const float* OD_plus, const float* OD_minus, int64_t ld, double fd_step,
                           const float* K, int n_spec, const float* tau, int64_t ld_tau, const rtx_grid* grid, int n_layers,
                           const double* T_h, int n_alt, const uint8_t* mask_h, double mu, int n_down, int n_angle,
                           int return_od, int t_pos, const double* V_h, int n_vec, float* d_tau, float* d_Lu, float* d_Ld,
                           int64_t ld_out, void* stream) {
  const TudColumnIn c = {OD, OD_plus, OD_minus, ld, fd_step, K, n_spec, tau, ld_tau, grid, n_layers, T_h, n_alt, mask_h, mu,
                         n_down, n_angle, return_od, t_pos, false};
  return tud_jvp_run(c, V_h, n_vec, d_tau, d_Lu, d_Ld, ld_out, stream);
}

extern "C" int rtx_tud_jvp_dod(const float* OD, const float* dOD_dT, int64_t ld, const float* K, int n_spec, const float* tau,
                               int64_t ld_tau, const rtx_grid* grid, int n_layers, const double* T_h, int n_alt,
                               const uint8_t* mask_h, double mu, int n_down, int n_angle, int return_od, int t_pos,
                               const double* V_h, int n_vec, float* d_tau, float* d_Lu, float* d_Ld, int64_t ld_out,
                               void* stream) {
  const TudColumnIn c = {OD, dOD_dT, dOD_dT, ld, 0.5, K, n_spec, tau, ld_tau, grid, n_layers, T_h, n_alt, mask_h, mu,
                         n_down, n_angle, return_od, t_pos, true};
  return tud_jvp_run(c, V_h, n_vec, d_tau, d_Lu, d_Ld, ld_out, stream);
}
