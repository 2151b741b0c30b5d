// Jacobian of the TUD outputs (tau, L-up per sensor altitude, Ld) with respect to layer temperatures and mixing ratios:
// the chain rule through the recurrences of rtx_tud, closed form.
//
// rtx_tud_jacobian : J[wrt][layer][row][nu], row = tau of each altitude, L-up of each altitude, Ld (2 n_alt + 1 rows);
//                    wrt = T (when asked, at t_pos) and one entry per species. The caller supplies, per layer, what the
//                    layer's optical depth does: (OD+ - OD-) / 2h for T, the line-sum at 1 ppmv for a species.
//
// Mapping (CDNA4): lane <-> wavenumber as in rtx_tud; a run-time loop over the layers; every J row is a dword store per
// lane, contiguous along the wavenumber axis (256 B per wave and store), non-temporal (nothing reads J back soon).
// The requested layers are taken TUDJ_CH at a time; for each such chunk the lane
//   (a) sweeps the column bottom-up once: fp64 prefix sums S_j = sum_{i<j} OD_i, D_l = B_l - L^(l-1) (L: the upwelling
//       recurrence) and the sums S_cnt(a) at each altitude's layer count;
//   (b) runs the downwelling stream recurrences top-down, TUDJ_QG streams at a time, from n_down - 1 to the chunk's
//       lowest layer, carrying E_{l,q} = B_l - R_{l+1,q} (R_{l+1,q}: the radiance arriving at the top of layer l);
//   (c) stores the chunk's rows.
// Every product of transmittances is exp(-(S_b - S_a) c) of an fp64 difference of prefix sums (no division of cumulative
// products, which underflow in opaque columns). The two differences a layer's sensitivity carries, B_l - L^(l-1) and
// B_l - R_{l+1}, are recurrences of their own driven by fp64 differences of neighbouring layers' B: no radiance is
// subtracted from a Planck value (that cancels where temperature barely changes with height, e.g. an isothermal
// stratosphere), and no "everything above l" sum appears. A layer's value depends only on
// the layer, never on which chunk or launch it is computed in: results are bit-identical for any subset of layers and
// any blocking of them.
#include "rtx_tud_jac_common.h"  // limits, TudJacArgs and its host setup, the row factors' device functions

__global__ __launch_bounds__(256) void tud_jac_kernel(TudJacArgs a) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.g.n) return;  // no cross-lane work: dead lanes leave
  const int nL = a.n_layers;
  const float* __restrict__ od = a.OD + i;
  const double x = grid_x(a.g, a.g.offset + i);
  const double x100 = x * 100.0;
  const double c1x3 = RT_C1 * (x100 * x100 * x100) * 1e4;
  const int nrow = 2 * a.n_alt + 1;
  const int n_wrt = a.with_T + a.n_spec;

  for (int k0 = 0; k0 < a.n_lay; k0 += TUDJ_CH) {
    const int nk = min(TUDJ_CH, a.n_lay - k0);
    int lmax = -1, lmin_d = nL;
    for (int k = 0; k < nk; ++k) {
      const int l = a.lay[k0 + k];
      lmax = max(lmax, l);
      if (l < a.n_down) lmin_d = min(lmin_d, l);
    }
    // ---- (a) bottom-up: prefix sums, D_l = B_l - L^(l-1), S at each altitude's count. D is carried by its own
    //      recurrence D_{j+1} = t_j D_j + (B_{j+1} - B_j), D_0 = B_0, with the B differences in fp64: forming B_l - L^(l-1)
    //      from the radiance recurrence cancels where neighbouring layers have (nearly) the same temperature ----
    double S0[TUDJ_CH], S1[TUDJ_CH];
    float Dl[TUDJ_CH], odl[TUDJ_CH];
#pragma unroll
    for (int k = 0; k < TUDJ_CH; ++k) { S0[k] = S1[k] = 0.0; Dl[k] = odl[k] = 0.f; }
    double Scnt[TUDJ_MAX_ALT];
#pragma unroll
    for (int q = 0; q < TUDJ_MAX_ALT; ++q) Scnt[q] = 0.0;
    double S = 0.0;
    double Bc = planck_f64(c1x3, x, a.c2l2e_over_T[0]);
    float D = (float)Bc;
    for (int j = 0; j < nL; ++j) {
#pragma unroll
      for (int q = 0; q < TUDJ_MAX_ALT; ++q)
        if (q < a.n_alt && a.count[q] == j) Scnt[q] = S;
      const float o = od[(size_t)j * a.ld];
#pragma unroll
      for (int k = 0; k < TUDJ_CH; ++k)
        if (k < nk && a.lay[k0 + k] == j) { S0[k] = S; Dl[k] = D; odl[k] = o; }
      if (j < lmax) {  // D_{j+1} is needed up to D_lmax
        const double Bn = planck_f64(c1x3, x, a.c2l2e_over_T[j + 1]);
        D = fmaf(__builtin_amdgcn_exp2f(-(o * a.mu) * (float)LOG2E), D, (float)(Bn - Bc));
        Bc = Bn;
      }
      S += (double)o;
#pragma unroll
      for (int k = 0; k < TUDJ_CH; ++k)
        if (k < nk && a.lay[k0 + k] == j) S1[k] = S;
    }
#pragma unroll
    for (int q = 0; q < TUDJ_MAX_ALT; ++q)
      if (q < a.n_alt && a.count[q] == nL) Scnt[q] = S;

    // ---- (b) downwelling: g = sum_q (w_q/c_q) e^{-S_{l+1}/c_q} E_{l,q},  E_{l,q} = B_l - R_{l+1,q},
    //                       h = sum_q w_q (1 - t_{l,q}) e^{-S_l/c_q} dB_l.
    //      E by its own recurrence, top-down: E_{n_down-1} = B_{n_down-1}, E_{j-1} = t_{j,q} E_j + (B_{j-1} - B_j) ----
    float gLd[TUDJ_CH], hLd[TUDJ_CH];
#pragma unroll
    for (int k = 0; k < TUDJ_CH; ++k) { gLd[k] = 0.f; hLd[k] = 0.f; }
    if (lmin_d < a.n_down) {
      for (int q0 = 0; q0 < a.n_str; q0 += TUDJ_QG) {
        double Bt = planck_f64(c1x3, x, a.c2l2e_over_T[a.n_down - 1]);
        float E[TUDJ_QG];
#pragma unroll
        for (int q = 0; q < TUDJ_QG; ++q) E[q] = (float)Bt;
        for (int j = a.n_down - 1; j >= lmin_d; --j) {
          const float o = od[(size_t)j * a.ld];
#pragma unroll
          for (int k = 0; k < TUDJ_CH; ++k) {
            if (k < nk && a.lay[k0 + k] == j) {  // wave-uniform
              float B, dB;
              planck_dT(c1x3, x, a.c2l2e_over_T[j], B, dB);
              float g = gLd[k], h = hLd[k];
#pragma unroll
              for (int q = 0; q < TUDJ_QG; ++q) {
                if (q0 + q < a.n_str) {
                  const double ic = a.str_ic[q0 + q];
                  g += a.str_wc[q0 + q] * exp_neg(S1[k] * ic) * E[q];
                  h += a.str_w[q0 + q] * one_minus_exp_neg(o * (float)ic) * exp_neg(S0[k] * ic) * dB;
                }
              }
              gLd[k] = g;
              hLd[k] = h;
            }
          }
          if (j > lmin_d) {
            const double Bn = planck_f64(c1x3, x, a.c2l2e_over_T[j - 1]);
            const float dBn = (float)(Bn - Bt);
#pragma unroll
            for (int q = 0; q < TUDJ_QG; ++q)
              E[q] = fmaf(__builtin_amdgcn_exp2f(-(o * (float)a.str_ic[q0 + q]) * (float)LOG2E), E[q], dBn);
            Bt = Bn;
          }
        }
      }
    }

    // ---- (c) rows of the chunk: the row factors g = d row / d OD_l and h = d row / d T_l at fixed OD (register arrays
    //      indexed by unrolled constants only), then J = g dOD/dx (+ h for T), one wrt at a time ----
    const size_t wstride = (size_t)a.n_lay * nrow * a.ld_J;
#pragma unroll
    for (int k = 0; k < TUDJ_CH; ++k) {
      if (k < nk) {
        const int l = a.lay[k0 + k];
        float B, dB;
        planck_dT(c1x3, x, a.c2l2e_over_T[l], B, dB);
        const float em_l = one_minus_exp_neg(odl[k] * a.mu);
        const float t_l = __builtin_amdgcn_exp2f(-(odl[k] * a.mu) * (float)LOG2E);  // not 1 - em_l: t is tiny where thick
        float gT[TUDJ_MAX_ALT], gU[TUDJ_MAX_ALT], hU[TUDJ_MAX_ALT];
        const unsigned lb = a.lbits[l];  // one scalar word per layer instead of 2 x n_alt table reads
#pragma unroll
        for (int ia = 0; ia < TUDJ_MAX_ALT; ++ia) {
          gT[ia] = gU[ia] = hU[ia] = 0.f;
          if (ia < a.n_alt) {
            // tau: -mu tau [Z_l <= zs]; returnOD: mu [Z_l <= zs]
            if ((lb >> ia) & 1u) gT[ia] = a.return_od ? a.mu : -a.mu * a.tau[(size_t)ia * a.ld_tau + i];
            // L-up: mu t_l Q D_l (D_l = B_l - L^(l-1)) and (1 - t_l) Q dB_l, Q = prod_{l<j<count} t_j; zero above the count
            if ((lb >> (16 + ia)) & 1u) {
              const float Q = exp_neg(a.mu_d * (Scnt[ia] - S1[k]));
              gU[ia] = a.mu * t_l * Q * Dl[k];
              hU[ia] = em_l * Q * dB;
            }
          }
        }
        // N_angle = 1: no stream has weight, compute_TUD's Ld is 0/0 (NaN), and so is its derivative in every layer
        const bool down = l < a.n_down;
        const float gD = a.n_str == 0 ? NAN : down ? gLd[k] : 0.f, hD = a.n_str == 0 ? NAN : down ? hLd[k] : 0.f;
        float* const out0 = a.J + (size_t)(k0 + k) * nrow * a.ld_J + i;
        for (int w = 0; w < n_wrt; ++w) {
          const bool isT = a.with_T && w == 0;
          // output slot: T at t_pos, the species in their order around it
          const int slot = !a.with_T ? w : isT ? a.t_pos : (w - 1 < a.t_pos ? w - 1 : w);
          float* const out = out0 + (size_t)slot * wstride;
          const size_t e = (size_t)l * a.ld + i;
          const float d = isT ? (a.ODp[e] - a.ODm[e]) * a.inv_2h : a.K[(size_t)(w - a.with_T) * nL * a.ld + e];
#pragma unroll
          for (int ia = 0; ia < TUDJ_MAX_ALT; ++ia)
            if (ia < a.n_alt) __builtin_nontemporal_store(gT[ia] * d, out + (size_t)ia * a.ld_J);
#pragma unroll
          for (int ia = 0; ia < TUDJ_MAX_ALT; ++ia)
            if (ia < a.n_alt)
              __builtin_nontemporal_store(isT ? fmaf(gU[ia], d, hU[ia]) : gU[ia] * d, out + (size_t)(a.n_alt + ia) * a.ld_J);
          __builtin_nontemporal_store(isT ? fmaf(gD, d, hD) : gD * d, out + (size_t)(2 * a.n_alt) * a.ld_J);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// Zeros for the *_dod entry points (rtx_tud_jac_common.h).
#include <mutex>
int rtx_tud_zero_rows(size_t count, const float** out) {
  struct Zeros { int dev; DevBuf<float> z; };
  static std::mutex mu;
  static std::vector<Zeros>* all = new std::vector<Zeros>();  // never destroyed: no device call from a static destructor
  int dev = 0;
  RTX_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  Zeros* e = nullptr;
  for (Zeros& c : *all)
    if (c.dev == dev) e = &c;
  if (!e) {
    all->emplace_back();
    e = &all->back();
    e->dev = dev;
  }
  if (count > e->z.cap()) {  // growth frees first, which waits for the kernels that read the old array
    if (e->z.reserve(count)) return 1;
    RTX_HIP(hipMemset(e->z.get(), 0, count * sizeof(float)));
  }
  *out = e->z.get();
  return 0;
}

static int tud_jacobian_run(const TudColumnIn& c, const int32_t* layers_h, int n_lay, float* J, int64_t ld_J, void* stream) {
  if (tud_column_check(c)) return 1;
  if (!J) RTX_FAIL("a required pointer is NULL");
  TudJacArgs a;
  if (tud_jac_setup(a, c, true, layers_h, n_lay)) return 1;
  if (ld_J < c.grid->n) RTX_FAIL("leading dimension smaller than the shard");
  a.J = J; a.ld_J = ld_J;
  if (c.grid->n == 0) return 0;
  unsigned blocks;
  if (tud_blocks(c.grid, 256, &blocks)) return 1;
  hipLaunchKernelGGL(tud_jac_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  RTX_LAUNCH_CHECK();
  return 0;
}

extern "C" int rtx_tud_jacobian(const float* OD, const float* OD_plus, const float* OD_minus, int64_t ld, double fd_step,
                                const float* K, int n_spec, const float* tau, int64_t ld_tau, const rtx_grid* grid, int n_layers,
                                const double* T_h, int n_alt, const uint8_t* mask_h, double mu, int n_down, int n_angle,
                                int return_od, const int32_t* layers_h, int n_lay, int t_pos, float* J, int64_t ld_J,
                                void* stream) {
  const TudColumnIn c = {OD, OD_plus, OD_minus, ld, fd_step, K, n_spec, tau, ld_tau, grid, n_layers, T_h, n_alt, mask_h, mu,
                         n_down, n_angle, return_od, t_pos, false};
  return tud_jacobian_run(c, layers_h, n_lay, J, ld_J, stream);
}

extern "C" int rtx_tud_jacobian_dod(const float* OD, const float* dOD_dT, int64_t ld, const float* K, int n_spec, const float* tau,
                                    int64_t ld_tau, const rtx_grid* grid, int n_layers, const double* T_h, int n_alt,
                                    const uint8_t* mask_h, double mu, int n_down, int n_angle, int return_od,
                                    const int32_t* layers_h, int n_lay, int t_pos, float* J, int64_t ld_J, void* stream) {
  const TudColumnIn c = {OD, dOD_dT, dOD_dT, ld, 0.5, K, n_spec, tau, ld_tau, grid, n_layers, T_h, n_alt, mask_h, mu,
                         n_down, n_angle, return_od, t_pos, true};
  return tud_jacobian_run(c, layers_h, n_lay, J, ld_J, stream);
}
