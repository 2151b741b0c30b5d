// Adjoint of the TUD Jacobian: out[v][wrt][layer] = sum_nu sum_row G[v][row][nu] J[wrt][layer][row][nu]
// with J what rtx_tud_jacobian defines, for cotangent vectors G on the rows tau / L-up per altitude / Ld. J is never stored.
//
// rtx_tud_vjp : the per-lane row factors g = d row / d OD_l and h = d row / d T_l are formed exactly as tud_jac_kernel forms
//               them (same sweeps, same device functions, fp32); where that kernel stores g dOD/dx (+ h), this one forms
//                 A_v = sum_row G_v,row g_row,  B_v = sum_row G_v,row h_row,  value = A_v dOD/dx (+ B_v for T)
//               in fp64 and reduces `value` over the wavenumbers at once.
//
// Mapping (CDNA4): lane <-> wavenumber and TUDJ_CH requested layers per chunk, as tud_jac_kernel. A row group without a
// cotangent is compiled out (template flags): no Ld cotangent -> no downwelling sweeps; no L-up and no Ld cotangent -> no
// Planck work and no bottom-up sweep; no tau cotangent -> tau is not read.
// Reduction, in a fixed order and without atomics:
//   1. each (layer, wrt, vector) value is summed over the wave's 64 lanes by an xor butterfly as soon as it is formed
//      (lanes past the shard hold 0): no per-layer accumulators stay in registers;
//   2. the four waves' sums meet in LDS and are added in wave order: one partial per workgroup of 256 wavenumbers,
//      part[workgroup][vector][wrt][layer] in device scratch;
//   3. tud_vjp_sum_kernel adds the partials of each output element in workgroup order.
// Which wavenumbers meet in which partial depends on grid->n alone, and a layer's per-lane value on the layer alone:
// out[v][w][k] is bit-identical for any subset, order or blocking of layers and vectors.
#include "rtx_tud_jac_common.h"

#define TUDV_NV 4  // cotangent vectors per launch: they share the sweeps; the LDS staging below grows with them
#define TUDV_MAX_WRT (TUDJ_MAX_SPEC + 1)
#define TUDV_WAVES 4

struct TudVjpArgs {
  TudJacArgs c;        // the column and the request (J unused)
  const float* G_tau;  // [nv][n_alt][ld_G] or NULL
  const float* G_Lu;   // [nv][n_alt][ld_G] or NULL
  const float* G_Ld;   // [nv][ld_G] or NULL
  long long ld_G;
  double* part;        // [workgroups][nv][n_wrt][n_lay]
  int nv;
};
static_assert(sizeof(TudVjpArgs) <= 4096, "kernel arguments are limited to 4 KiB");

__device__ __forceinline__ double wave_sum(double v) {  // every lane gets the same bits
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

template <bool TAU, bool LU, bool LD>
__global__ __launch_bounds__(256) void tud_vjp_kernel(TudVjpArgs v) {
  const TudJacArgs& a = v.c;
  __shared__ double red[TUDV_WAVES][TUDV_NV * TUDV_MAX_WRT * TUDJ_CH];
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i0 < a.g.n;
  const long long i = live ? i0 : a.g.n - 1;  // lanes past the shard stay for the cross-lane sums and contribute 0
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nL = a.n_layers;
  const float* __restrict__ od = a.OD + i;
  const double x = grid_x(a.g, a.g.offset + i);
  const double x100 = x * 100.0;
  const double c1x3 = RT_C1 * (x100 * x100 * x100) * 1e4;
  const int n_wrt = a.with_T + a.n_spec;
  const size_t gstride = (size_t)a.n_alt * v.ld_G;  // one vector of G_tau / G_Lu

  for (int k0 = 0; k0 < a.n_lay; k0 += TUDJ_CH) {
    const int nk = min(TUDJ_CH, a.n_lay - k0);
    int lmax = -1, lmin_d = nL;
    for (int k = 0; k < nk; ++k) {
      const int l = a.lay[k0 + k];
      lmax = max(lmax, l);
      if (l < a.n_down) lmin_d = min(lmin_d, l);
    }
    // ---- (a) bottom-up, as tud_jac_kernel: prefix sums, D_l = B_l - L^(l-1) (L-up only), S at each altitude's count ----
    double S0[TUDJ_CH], S1[TUDJ_CH];
    float Dl[TUDJ_CH], odl[TUDJ_CH];
#pragma unroll
    for (int k = 0; k < TUDJ_CH; ++k) { S0[k] = S1[k] = 0.0; Dl[k] = odl[k] = 0.f; }
    double Scnt[TUDJ_MAX_ALT];
#pragma unroll
    for (int q = 0; q < TUDJ_MAX_ALT; ++q) Scnt[q] = 0.0;
    if constexpr (LU || LD) {
      double S = 0.0;
      double Bc = 0.0;
      float D = 0.f;
      if constexpr (LU) {
        Bc = planck_f64(c1x3, x, a.c2l2e_over_T[0]);
        D = (float)Bc;
      }
      for (int j = 0; j < nL; ++j) {
        if constexpr (LU) {
#pragma unroll
          for (int q = 0; q < TUDJ_MAX_ALT; ++q)
            if (q < a.n_alt && a.count[q] == j) Scnt[q] = S;
        }
        const float o = od[(size_t)j * a.ld];
#pragma unroll
        for (int k = 0; k < TUDJ_CH; ++k)
          if (k < nk && a.lay[k0 + k] == j) { S0[k] = S; Dl[k] = D; odl[k] = o; }
        if constexpr (LU) {
          if (j < lmax) {  // D_{j+1} is needed up to D_lmax
            const double Bn = planck_f64(c1x3, x, a.c2l2e_over_T[j + 1]);
            D = fmaf(__builtin_amdgcn_exp2f(-(o * a.mu) * (float)LOG2E), D, (float)(Bn - Bc));
            Bc = Bn;
          }
        }
        S += (double)o;
#pragma unroll
        for (int k = 0; k < TUDJ_CH; ++k)
          if (k < nk && a.lay[k0 + k] == j) S1[k] = S;
      }
      if constexpr (LU) {
#pragma unroll
        for (int q = 0; q < TUDJ_MAX_ALT; ++q)
          if (q < a.n_alt && a.count[q] == nL) Scnt[q] = S;
      }
    }

    // ---- (b) downwelling, as tud_jac_kernel; not compiled without a cotangent on Ld ----
    float gLd[TUDJ_CH], hLd[TUDJ_CH];
#pragma unroll
    for (int k = 0; k < TUDJ_CH; ++k) { gLd[k] = 0.f; hLd[k] = 0.f; }
    if constexpr (LD) {
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
    }

    // ---- (c) the chunk's row factors (tud_jac_kernel's), contracted with G over the rows and summed over the wave ----
#pragma unroll
    for (int k = 0; k < TUDJ_CH; ++k) {
      if (k < nk) {
        const int l = a.lay[k0 + k];
        float B = 0.f, dB = 0.f;
        if constexpr (LU || LD) planck_dT(c1x3, x, a.c2l2e_over_T[l], B, dB);
        const float em_l = one_minus_exp_neg(odl[k] * a.mu);
        const float t_l = __builtin_amdgcn_exp2f(-(odl[k] * a.mu) * (float)LOG2E);
        float gU[TUDJ_MAX_ALT], hU[TUDJ_MAX_ALT];
        const unsigned lb = a.lbits[l];
#pragma unroll
        for (int ia = 0; ia < TUDJ_MAX_ALT; ++ia) {
          gU[ia] = hU[ia] = 0.f;
          if (ia < a.n_alt) {
            if constexpr (LU) {
              if ((lb >> (16 + ia)) & 1u) {
                const float Q = exp_neg(a.mu_d * (Scnt[ia] - S1[k]));
                gU[ia] = a.mu * t_l * Q * Dl[k];
                hU[ia] = em_l * Q * dB;
              }
            }
          }
        }
        const bool down = l < a.n_down;
        const float gD = a.n_str == 0 ? NAN : down ? gLd[k] : 0.f, hD = a.n_str == 0 ? NAN : down ? hLd[k] : 0.f;
        const size_t e = (size_t)l * a.ld + i;
        for (int vv = 0; vv < v.nv; ++vv) {
          double A = 0.0, Bv = 0.0;  // sum_row G g, sum_row G h: fp64 products of fp32 factors
          if constexpr (TAU) {
            const float* __restrict__ G = v.G_tau + (size_t)vv * gstride + i;
#pragma unroll
            for (int ia = 0; ia < TUDJ_MAX_ALT; ++ia)
              if (ia < a.n_alt && ((lb >> ia) & 1u)) {  // tau: -mu tau [Z_l <= zs]; returnOD: mu [Z_l <= zs]
                const float gT = a.return_od ? a.mu : -a.mu * a.tau[(size_t)ia * a.ld_tau + i];  // formed here: no array kept
                A += (double)G[(size_t)ia * v.ld_G] * (double)gT;
              }
          }
          if constexpr (LU) {
            const float* __restrict__ G = v.G_Lu + (size_t)vv * gstride + i;
#pragma unroll
            for (int ia = 0; ia < TUDJ_MAX_ALT; ++ia) {
              if (ia < a.n_alt) {
                const double Gd = (double)G[(size_t)ia * v.ld_G];
                A += Gd * (double)gU[ia];
                Bv += Gd * (double)hU[ia];
              }
            }
          }
          if constexpr (LD) {
            const double Gd = (double)v.G_Ld[(size_t)vv * v.ld_G + i];
            A += Gd * (double)gD;
            Bv += Gd * (double)hD;
          }
          for (int w = 0; w < n_wrt; ++w) {
            const bool isT = a.with_T && w == 0;
            // output slot: T at t_pos, the species in their order around it
            const int slot = !a.with_T ? w : isT ? a.t_pos : (w - 1 < a.t_pos ? w - 1 : w);
            const float d = isT ? (a.ODp[e] - a.ODm[e]) * a.inv_2h : a.K[(size_t)(w - a.with_T) * nL * a.ld + e];
            double val = A * (double)d;
            if (isT) val += Bv;
            val = wave_sum(live ? val : 0.0);
            if (lane == 0) red[wave][(vv * n_wrt + slot) * TUDJ_CH + k] = val;
          }
        }
      }
    }
    // ---- the workgroup's partial of this chunk: the four waves in wave order ----
    __syncthreads();
    const int per_v = n_wrt * TUDJ_CH;
    for (int t = threadIdx.x; t < v.nv * per_v; t += blockDim.x) {
      const int k = t % TUDJ_CH;
      if (k < nk) {
        double s = red[0][t];
#pragma unroll
        for (int wv = 1; wv < TUDV_WAVES; ++wv) s += red[wv][t];
        const int vs = t / TUDJ_CH;  // vv * n_wrt + slot
        v.part[((size_t)blockIdx.x * v.nv * n_wrt + vs) * a.n_lay + k0 + k] = s;
      }
    }
    __syncthreads();
  }
}

// out[e] = sum over the workgroups' partials of element e, in workgroup order (loads eight ahead, adds in order)
__global__ __launch_bounds__(64) void tud_vjp_sum_kernel(const double* __restrict__ part, long long n_part, int n_out,
                                                          double* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_out) return;
  double s = 0.0;
  long long b = 0;
  for (; b + 8 <= n_part; b += 8) {
    double p[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) p[u] = part[(size_t)(b + u) * n_out + e];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += p[u];
  }
  for (; b < n_part; ++b) s += part[(size_t)b * n_out + e];
  out[e] = s;
}

// the partials, per (device, stream)
static StreamScratch* const vjp_scratch = new StreamScratch();

extern "C" int rtx_tud_vjp_max_vectors(void) { return TUDV_NV; }

static int tud_vjp_run(const TudColumnIn& c, const int32_t* layers_h, int n_lay, const float* G_tau, const float* G_Lu,
                       const float* G_Ld, int64_t ld_G, int n_vec, double* out, void* stream) {
  if (tud_column_check(c)) return 1;
  if (!out) RTX_FAIL("out is NULL");
  if (!G_tau && !G_Lu && !G_Ld) RTX_FAIL("no cotangent: G_tau, G_Lu and G_Ld are all NULL");
  if (n_vec < 1 || n_vec > TUDV_NV) RTX_FAIL("n_vec=%d outside [1,%d] (rtx_tud_vjp_max_vectors)", n_vec, TUDV_NV);
  TudVjpArgs v;
  if (tud_jac_setup(v.c, c, G_tau != nullptr, layers_h, n_lay)) return 1;
  if (ld_G < c.grid->n) RTX_FAIL("ld_G=%lld smaller than the shard", (long long)ld_G);
  hipStream_t st = (hipStream_t)stream;
  const int n_out = n_vec * (v.c.with_T + c.n_spec) * n_lay;
  if (c.grid->n == 0) {
    RTX_HIP(hipMemsetAsync(out, 0, (size_t)n_out * sizeof(double), st));
    return 0;
  }
  unsigned blocks;
  if (tud_blocks(c.grid, 64 * TUDV_WAVES, &blocks)) return 1;
  void* ws = nullptr;
  if (vjp_scratch->get(st, (size_t)blocks * n_out * sizeof(double), &ws)) return 1;
  v.G_tau = G_tau; v.G_Lu = G_Lu; v.G_Ld = G_Ld; v.ld_G = ld_G; v.part = (double*)ws; v.nv = n_vec;
  tud_dispatch_rows(G_tau, G_Lu, G_Ld, [&](auto tau, auto up, auto down) {
    hipLaunchKernelGGL((tud_vjp_kernel<decltype(tau)::value, decltype(up)::value, decltype(down)::value>), dim3(blocks),
                       dim3(64 * TUDV_WAVES), 0, st, v);
  });
  RTX_LAUNCH_CHECK();
  hipLaunchKernelGGL(tud_vjp_sum_kernel, dim3((unsigned)((n_out + 63) / 64)), dim3(64), 0, st, (const double*)ws, (long long)blocks,
                     n_out, out);
  RTX_LAUNCH_CHECK();
  return 0;
}

extern "C" int rtx_tud_vjp(const float* OD, const float* OD_plus, const float* OD_minus, int64_t ld, double fd_step,
                           const float* K, int n_spec, const float* tau, int64_t ld_tau, const rtx_grid* grid, int n_layers,
                           const double* T_h, int n_alt, const uint8_t* mask_h, double mu, int n_down, int n_angle,
                           int return_od, const int32_t* layers_h, int n_lay, int t_pos, const float* G_tau,
                           const float* G_Lu, const float* G_Ld, int64_t ld_G, int n_vec, double* out, void* stream) {
  const TudColumnIn c = {OD, OD_plus, OD_minus, ld, fd_step, K, n_spec, tau, ld_tau, grid, n_layers, T_h, n_alt, mask_h, mu,
                         n_down, n_angle, return_od, t_pos, false};
  return tud_vjp_run(c, layers_h, n_lay, G_tau, G_Lu, G_Ld, ld_G, n_vec, out, stream);
}

extern "C" int rtx_tud_vjp_dod(const float* OD, const float* dOD_dT, int64_t ld, const float* K, int n_spec, const float* tau,
                               int64_t ld_tau, const rtx_grid* grid, int n_layers, const double* T_h, int n_alt,
                               const uint8_t* mask_h, double mu, int n_down, int n_angle, int return_od, const int32_t* layers_h,
                               int n_lay, int t_pos, const float* G_tau, const float* G_Lu, const float* G_Ld, int64_t ld_G,
                               int n_vec, double* out, void* stream) {
  const TudColumnIn c = {OD, dOD_dT, dOD_dT, ld, 0.5, K, n_spec, tau, ld_tau, grid, n_layers, T_h, n_alt, mask_h, mu,
                         n_down, n_angle, return_od, t_pos, true};
  return tud_vjp_run(c, layers_h, n_lay, G_tau, G_Lu, G_Ld, ld_G, n_vec, out, stream);
}
