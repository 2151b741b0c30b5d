// Adjoint of the fused band radiances under response tables (include/radtxfr_hip.h, rtx_srf_radiance_vjp):
// the transpose of rtx_srf_moments + rtx_band_mix. With w = R_b(X_i) D_i, N_b = sum_i w, hat_j np.interp's hats on Xk and
//   L[t][b][e] = (1 / N_b) sum_i w [tau (eps_e B(nu_i, Ts_t) + (1 - eps_e) Ld) + La],  eps_e = sum_j hat_j E[j][e],
// a cotangent g[t][b][e] on L gives, over the live bands (N_b > 0) only,
//   H[t][b][j] = sum_e g[t][b][e] E[j][e]
//   A_t,i = sum_b (w / N_b) sum_j hat_j(nu_i) H[t][b][j],   S_i = sum_t sum_b (w / N_b) sum_e g[t][b][e]
//   G_tau = sum_t A_t (B_t - Ld) + S Ld,   G_La = S,   G_Ld = tau (S - sum_t A_t)
//   dTs[t] = sum_i A_t,i tau dB/dT(nu_i, Ts_t),   dE[j][e] = sum_t sum_b g[t][b][e] M[t][b][j] / N_b.
// Nothing of size nX * nE is formed, as in the forward.
//
// Structure: five small kernels around one pass over the points.
//   srfv_support_kernel  per band: support [lo, hi) on the grid and first / last emissivity knot touched (srfm_support_kernel's)
//   srfv_norm_kernel     per chunk of SRF_CH points: the chunk's sum of every reaching band's weights, in fp64, the weights
//                        and the order of the sum srfm_chunk_kernel's to the letter
//   srfv_nsum_kernel     per band: the chunk sums in ascending chunk order, rounded to fp32 as rtx_srf_moments stores N
//   srfv_h_kernel        per band: H on the knots the band touches and sum_t sum_e g, fp64 sums over e ascending
//   srfv_point_kernel    per chunk, ONE LANE PER POINT: the workgroup walks the bands that reach the chunk in ascending band
//                        index, stages each band's knots in LDS, and a lane adds S and A_t in fp64; then one Planck
//                        evaluation per (point, temperature) and the three rows. The dTs terms of a chunk are summed by an
//                        xor butterfly over the wave's 64 lanes, then over the 16 waves in wave order.
//   srfv_dts_kernel      dTs[t]: the chunks' partials in ascending chunk order
//   srfv_de_kernel       dE[j][e]: fp64 over (t, b) ascending, M from an rtx_srf_moments run inside the call
// No atomics. Determinism: see the header.
#include "rtx_srf_common.h"
#include "rtx_tud_jac_common.h"  // planck_dT

#define SRFV_MAXT 8    // temperatures per call: rtx_srf_moments_max_temps()
#define SRFV_GROUP 128  // bands per launch of the support kernel (their knot ranges travel as kernel arguments)

struct SrfvArgs {
  SrfArgs s;  // g, nx, kx, kr as in rtx_srf_moments; X = NULL (uniform grid), the rest unused
  const float *tau, *La, *Ld, *E, *g;
  const double* Xk;
  long long nk, nE;
  int nT, nB;
  double ct[SRFV_MAXT];  // 100 c2 log2(e) / Ts_t
  int g0, ng;            // the support kernel's group: bands [g0, g0 + ng)
  int ks[SRFV_GROUP + 1];
  int* ksd;              // [nB + 1] knot_start on the device (written by the support kernel)
  long long* sup;        // [nB][2]
  int2* jr;              // [nB]
  double* WN;            // [n_chunks][nB] chunk sums of the weights
  float* N;              // [nB]
  double* invN;          // [nB] 1 / N, 0 for a band that is not live
  double* SgT;           // [nB] sum_t sum_e g
  float* H;              // [nT][nB][nk], written on jrange only
  const float* M;        // [nT][nB][nk] rtx_srf_moments' (dE only)
  double* part;          // [n_chunks][nT] dTs partials
  float *Gt, *Ga, *Gd;
  double *dTs, *dE;
};

__global__ __launch_bounds__(SRFV_GROUP) void srfv_support_kernel(SrfvArgs a) {
  const int j = threadIdx.x;
  if (j >= a.ng) return;
  const int b = a.g0 + j;
  a.ksd[b] = a.ks[j];
  if (j == a.ng - 1) a.ksd[b + 1] = a.ks[j + 1];
  const double x_first = a.s.kx[a.ks[j]], x_last = a.s.kx[a.ks[j + 1] - 1];
  const long long lo = srf_bound(a.s, x_first, 0), hi = srf_bound(a.s, x_last, 1);
  a.sup[2 * b] = lo;
  a.sup[2 * b + 1] = hi;
  int2 jr = make_int2(0, -1);
  if (hi > lo) {
    const long long c0 = srfm_count(a.Xk, a.nk, srf_x(a.s, lo)), c1 = srfm_count(a.Xk, a.nk, srf_x(a.s, hi - 1));
    jr.x = (int)(c0 > 0 ? c0 - 1 : 0);
    jr.y = (int)(c1 < a.nk - 1 ? c1 : a.nk - 1);
  }
  a.jr[b] = jr;
}

// the rows [lo, hi) of chunk [r0, r1) under band b, counted from r0; empty: false
__device__ __forceinline__ bool srfv_reach(const SrfvArgs& a, int b, long long r0, long long r1, int& lo, int& hi) {
  const long long L = a.sup[2 * b], H = a.sup[2 * b + 1];
  const long long l = L > r0 ? L : r0, h = H < r1 ? H : r1;
  if (h <= l) return false;
  lo = (int)(l - r0); hi = (int)(h - r0);
  return true;
}

// stages the knots of band b that lie under rows [lo, hi) of the chunk, as srf_rows_kernel does; returns their number
__device__ __forceinline__ int srfv_stage(const SrfvArgs& a, int b, long long r0, int lo, int hi, double* s_kx, float* s_kr, int nthreads) {
  const int k0 = a.ksd[b], nkb = a.ksd[b + 1] - k0;
  const double* kx = a.s.kx + k0;
  const int jA = srf_segment(kx, nkb, srf_x(a.s, r0 + lo));
  const int m = srf_segment(kx, nkb, srf_x(a.s, r0 + hi - 1)) + 2 - jA;  // knots jA .. jB + 1
  for (int q = threadIdx.x; q < m; q += nthreads) { s_kx[q] = kx[jA + q]; s_kr[q] = a.s.kr[k0 + jA + q]; }
  return m;
}

// N's chunk sums: srfm_chunk_kernel's weights and its order (a thread's four rows, the lanes of a wave, the four waves)
__global__ __launch_bounds__(256) void srfv_norm_kernel(SrfvArgs a) {
  const long long chunk = blockIdx.x;
  const long long r0 = chunk * SRF_CH, r1 = r0 + SRF_CH < a.s.nx ? r0 + SRF_CH : a.s.nx;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ float s_w[SRF_CH];
  __shared__ double s_kx[SRF_MAX_KNOTS];
  __shared__ float s_kr[SRF_MAX_KNOTS];
  __shared__ double s_red[4];
  for (int b = 0; b < a.nB; ++b) {
    int lo, hi;
    if (!srfv_reach(a, b, r0, r1, lo, hi)) continue;  // uniform over the workgroup
    const int m = srfv_stage(a, b, r0, lo, hi, s_kx, s_kr, 256);
    __syncthreads();
    int seg = 0;
    for (int t = threadIdx.x; t < SRF_CH; t += 256)
      s_w[t] = t >= lo && t < hi ? srf_weight(a.s, s_kx, s_kr, m, seg, r0 + t) : 0.f;
    __syncthreads();
    double n = 0.0;
    for (int t = threadIdx.x; t < SRF_CH; t += 256) {
      const double w = (double)s_w[t];
      if (w != 0.0) n += w;
    }
    for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off);
    if (lane == 0) s_red[wave] = n;
    __syncthreads();
    if (threadIdx.x == 0) a.WN[chunk * a.nB + b] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
    __syncthreads();  // s_w, the knots and s_red are rewritten by the next band
  }
}

__global__ __launch_bounds__(256) void srfv_nsum_kernel(SrfvArgs a) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= a.nB) return;
  const long long lo = a.sup[2 * b], hi = a.sup[2 * b + 1];
  double N = 0.0;
  if (hi > lo)
    for (long long ch = lo / SRF_CH; ch <= (hi - 1) / SRF_CH; ++ch) N += a.WN[ch * a.nB + b];
  const float Nf = (float)N;  // what rtx_srf_moments stores and rtx_band_mix divides by
  a.N[b] = Nf;
  if (a.invN) a.invN[b] = Nf > 0.f ? 1.0 / (double)Nf : 0.0;
}

// one workgroup per band: H[t][b][j] on jrange[b] (fp64 over e ascending, stored fp32) and SgT[b] = sum_t sum_e g[t][b][e]
// (a thread's e = tid, tid + 256, ... for t ascending, then the 256 threads in order). A band that is not live gets SgT = 0
// and no H: its g is never read, whatever it holds.
__global__ __launch_bounds__(256) void srfv_h_kernel(SrfvArgs a) {
  const int b = blockIdx.x;
  __shared__ double s_p[256];
  const bool live = a.invN[b] > 0.0;
  if (!live) {
    if (threadIdx.x == 0) a.SgT[b] = 0.0;
    return;
  }
  double p = 0.0;
  for (int t = 0; t < a.nT; ++t) {
    const float* g = a.g + ((size_t)t * a.nB + b) * (size_t)a.nE;
    for (long long e = threadIdx.x; e < a.nE; e += 256) p += (double)g[e];
  }
  s_p[threadIdx.x] = p;
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = 0.0;
    for (int q = 0; q < 256; ++q) v += s_p[q];
    a.SgT[b] = v;
  }
  const int2 jr = a.jr[b];
  const long long nj = (long long)jr.y - jr.x + 1;
  for (long long q = threadIdx.x; q < nj * a.nT; q += 256) {
    const int t = (int)(q / nj);
    const long long j = jr.x + (q - (long long)t * nj);
    const float* g = a.g + ((size_t)t * a.nB + b) * (size_t)a.nE;
    const float* E = a.E + (size_t)j * (size_t)a.nE;
    double h = 0.0;
    for (long long e = 0; e < a.nE; ++e) h += (double)g[e] * (double)E[e];
    a.H[((size_t)t * a.nB + b) * (size_t)a.nk + j] = (float)h;
  }
}

__device__ __forceinline__ double srfv_wave_sum(double v) {
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__global__ __launch_bounds__(SRF_CH) void srfv_point_kernel(SrfvArgs a) {
  const long long chunk = blockIdx.x;
  const long long r0 = chunk * SRF_CH, r1 = r0 + SRF_CH < a.s.nx ? r0 + SRF_CH : a.s.nx;
  const int p = threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long i = r0 + p;
  const bool valid = i < r1;
  __shared__ double s_kx[SRF_MAX_KNOTS];
  __shared__ float s_kr[SRF_MAX_KNOTS];
  __shared__ double s_red[SRFV_MAXT][SRF_CH / 64];
  // the point's knot interval and its weight on the upper knot, as srfm_chunk_kernel forms them
  double x = 0.0;
  long long j0 = 0;
  float f0 = 1.f, f = 0.f;
  if (valid) {
    x = srf_x(a.s, i);
    const long long cnt = srfm_count(a.Xk, a.nk, x);
    j0 = cnt > 0 ? cnt - 1 : 0;
    if (cnt > 0 && cnt < a.nk) srfm_hats(x, a.Xk[cnt - 1], a.Xk[cnt], f0, f);
  }
  const double h0 = (double)f0, h1 = (double)f;
  double S = 0.0, A[SRFV_MAXT];
#pragma unroll
  for (int t = 0; t < SRFV_MAXT; ++t) A[t] = 0.0;
  bool any = false;
  for (int b = 0; b < a.nB; ++b) {
    int lo, hi;
    if (!srfv_reach(a, b, r0, r1, lo, hi)) continue;  // uniform over the workgroup
    const double inv = a.invN[b];
    if (!(inv > 0.0)) continue;  // not live: contributes nothing
    const int m = srfv_stage(a, b, r0, lo, hi, s_kx, s_kr, SRF_CH);
    __syncthreads();
    if (p >= lo && p < hi) {
      int u = 1, v = m - 1;  // the segment srf_weight's walk from 0 would reach: the knots 1 .. m - 2 that are <= x
      while (u < v) {
        const int mid = (u + v) >> 1;
        if (x >= s_kx[mid]) u = mid + 1; else v = mid;
      }
      int seg = u - 1;
      const float w = srf_weight(a.s, s_kx, s_kr, m, seg, i);
      if (w != 0.f) {  // a row of weight 0 is skipped, as in the forward
        any = true;
        const double c = (double)w * inv;
        S += c * a.SgT[b];
#pragma unroll
        for (int t = 0; t < SRFV_MAXT; ++t) {
          if (t < a.nT) {
            const float* H = a.H + ((size_t)t * a.nB + b) * (size_t)a.nk + j0;
            double h = h0 * (double)H[0];
            if (f != 0.f) h += h1 * (double)H[1];
            A[t] += c * h;
          }
        }
      }
    }
    __syncthreads();  // the knots are rewritten by the next band
  }
  // ---- the three rows and the dTs terms: one Planck evaluation per (point, temperature)
  double term[SRFV_MAXT];
#pragma unroll
  for (int t = 0; t < SRFV_MAXT; ++t) term[t] = 0.0;
  if (valid) {
    float gt = 0.f, ga = 0.f, gd = 0.f;  // a point under no live band: exact zeros
    if (any) {
      const double tt = (double)a.tau[i], ld = (double)a.Ld[i];
      double sumA = 0.0, acc = 0.0;
      if (a.Gt || a.dTs) {
        const double x100 = x * 100.0;
        const double c1x3 = RT_C1 * (x100 * x100 * x100) * 1e4;
#pragma unroll
        for (int t = 0; t < SRFV_MAXT; ++t) {
          if (t < a.nT) {
            float B, dB;
            planck_dT(c1x3, x, a.ct[t], B, dB);
            acc += A[t] * ((double)B - ld);
            term[t] = A[t] * tt * (double)dB;
          }
        }
      }
#pragma unroll
      for (int t = 0; t < SRFV_MAXT; ++t)
        if (t < a.nT) sumA += A[t];
      gt = (float)(acc + S * ld);
      ga = (float)S;
      gd = (float)(tt * (S - sumA));
    }
    if (a.Gt) a.Gt[i] = gt;
    if (a.Ga) a.Ga[i] = ga;
    if (a.Gd) a.Gd[i] = gd;
  }
  if (a.dTs) {  // uniform
#pragma unroll
    for (int t = 0; t < SRFV_MAXT; ++t) {
      if (t < a.nT) {
        const double v = srfv_wave_sum(term[t]);
        if (lane == 0) s_red[t][wave] = v;
      }
    }
    __syncthreads();
    if (p < a.nT) {
      double v = 0.0;
      for (int w = 0; w < SRF_CH / 64; ++w) v += s_red[p][w];
      a.part[chunk * a.nT + p] = v;
    }
  }
}

__global__ __launch_bounds__(64) void srfv_dts_kernel(SrfvArgs a, long long n_chunks) {
  const int t = threadIdx.x;
  if (t >= a.nT) return;
  double v = 0.0;
  for (long long ch = 0; ch < n_chunks; ++ch) v += a.part[ch * a.nT + t];
  a.dTs[t] = v;
}

// one thread per (knot j = blockIdx.x, column e): (t, b) ascending in fp64; a band that does not touch knot j holds M = 0
// there and is skipped, a band that is not live is skipped whatever its g holds
__global__ __launch_bounds__(256) void srfv_de_kernel(SrfvArgs a) {
  const long long j = blockIdx.x, e = (long long)blockIdx.y * 256 + threadIdx.x;
  if (e >= a.nE) return;
  double acc = 0.0;
  for (int t = 0; t < a.nT; ++t) {
    for (int b = 0; b < a.nB; ++b) {
      const int2 jr = a.jr[b];
      const double inv = a.invN[b];
      if (j < jr.x || j > jr.y || !(inv > 0.0)) continue;  // uniform over the workgroup
      const size_t tb = (size_t)t * a.nB + b;
      acc += (double)a.g[tb * (size_t)a.nE + e] * ((double)a.M[tb * (size_t)a.nk + j] * inv);
    }
  }
  a.dE[(size_t)j * (size_t)a.nE + e] = acc;
}

// workspace per (device, stream), as rtx_srf_apply's
static StreamScratch* const srfv_scratch = new StreamScratch();

static int srfv_check_bands(const rtx_grid* grid, int nB, const int32_t* knot_start_h) {
  if (!grid) RTX_FAIL("no grid");
  if (rtx_check_grid(grid)) return 1;
  if (nB < 0) RTX_FAIL("negative size");
  if (nB == 0) return 0;
  if (!knot_start_h) RTX_FAIL("a required pointer is NULL");
  if (knot_start_h[0] < 0) RTX_FAIL("knot_start[0]=%d is negative", (int)knot_start_h[0]);
  for (int b = 0; b < nB; ++b) {
    const long long n = (long long)knot_start_h[b + 1] - (long long)knot_start_h[b];
    if (n < 0) RTX_FAIL("knot_start is not ascending at band %d", b);
    if (n < 2) RTX_FAIL("band %d has %lld knots: a response table needs at least 2", b, n);
    if (n > SRF_MAX_KNOTS) RTX_FAIL("band %d has %lld knots: at most %d", b, n, SRF_MAX_KNOTS);
  }
  const long long n_chunks = (grid->n + SRF_CH - 1) / SRF_CH;
  if (n_chunks > 0x7fffffffLL / (SRF_CH / 64)) RTX_FAIL("grid->n=%lld: too many chunks", (long long)grid->n);
  return 0;
}

// carves the workspace: every array 16-byte aligned
struct SrfvCarve {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t at = off;
    off += (bytes + 15) & ~(size_t)15;
    return at;
  }
};

// supports, chunk sums and N (invN, when a.invN is set) of all bands: three kinds of launch
static int srfv_norms(SrfvArgs& a, const int32_t* knot_start_h, long long n_chunks, hipStream_t st) {
  for (int g0 = 0; g0 < a.nB; g0 += SRFV_GROUP) {
    a.g0 = g0;
    a.ng = a.nB - g0 < SRFV_GROUP ? a.nB - g0 : SRFV_GROUP;
    for (int j = 0; j <= SRFV_GROUP; ++j) a.ks[j] = knot_start_h[g0 + (j < a.ng ? j : a.ng)];
    hipLaunchKernelGGL(srfv_support_kernel, dim3(1), dim3(SRFV_GROUP), 0, st, a);
    RTX_LAUNCH_CHECK();
  }
  if (n_chunks > 0) {
    hipLaunchKernelGGL(srfv_norm_kernel, dim3((unsigned)n_chunks), dim3(256), 0, st, a);
    RTX_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(srfv_nsum_kernel, dim3((unsigned)((a.nB + 255) / 256)), dim3(256), 0, st, a);
  RTX_LAUNCH_CHECK();
  return 0;
}

static void srfv_base(SrfvArgs& a, const rtx_grid* grid, const double* knot_x_d, const float* knot_r_d, int nB) {
  memset(&a, 0, sizeof(a));
  a.s.g = to_dev(grid);
  a.s.nx = grid->n;
  a.s.kx = knot_x_d; a.s.kr = knot_r_d;
  a.nB = nB;
  a.nk = 1; a.nT = 0;
}

extern "C" int rtx_srf_norms(const rtx_grid* grid, int nB, const int32_t* knot_start_h, const double* knot_x_d, const float* knot_r_d,
                             float* N_out, void* stream) {
  if (srfv_check_bands(grid, nB, knot_start_h)) return 1;
  if (nB == 0) return 0;
  if (!knot_x_d || !knot_r_d || !N_out) RTX_FAIL("a required pointer is NULL");
  hipStream_t st = (hipStream_t)stream;
  const long long n_chunks = (grid->n + SRF_CH - 1) / SRF_CH;
  SrfvCarve c;
  const size_t o_sup = c.take((size_t)nB * 2 * sizeof(long long)), o_jr = c.take((size_t)nB * sizeof(int2)),
               o_ks = c.take(((size_t)nB + 1) * sizeof(int)), o_wn = c.take((size_t)n_chunks * nB * sizeof(double)),
               o_xk = c.take(sizeof(double));
  char* base = nullptr;
  if (srfv_scratch->get(st, c.off, (void**)&base)) return 1;
  SrfvArgs a;
  srfv_base(a, grid, knot_x_d, knot_r_d, nB);
  a.sup = (long long*)(base + o_sup); a.jr = (int2*)(base + o_jr); a.ksd = (int*)(base + o_ks); a.WN = (double*)(base + o_wn);
  // the support kernel also finds the emissivity knots a band touches: here one knot, wherever it lies
  a.Xk = (const double*)(base + o_xk);
  RTX_HIP(hipMemsetAsync(base + o_xk, 0, sizeof(double), st));
  a.N = N_out;
  return srfv_norms(a, knot_start_h, n_chunks, st);
}

extern "C" int rtx_srf_radiance_vjp(const rtx_grid* grid, const float* tau, const float* La, const float* Ld, const double* Ts_h, int nT,
                                    const double* Xk, int64_t nk, int nB, const int32_t* knot_start_h, const double* knot_x_d,
                                    const float* knot_r_d, const float* E, int64_t nE, const float* g, float* G_tau, float* G_La,
                                    float* G_Ld, double* dTs, double* dE, void* stream) {
  if (!grid) RTX_FAIL("no grid");
  if (rtx_check_grid(grid)) return 1;
  if (nk < 1) RTX_FAIL("nk=%lld: need at least 1 emissivity knot", (long long)nk);
  if (nk > (1ll << 23)) RTX_FAIL("nk=%lld: at most %lld emissivity knots", (long long)nk, 1ll << 23);
  if (nT < 1 || nT > SRFV_MAXT || nT > rtx_srf_moments_max_temps()) RTX_FAIL("nT=%d outside [1,%d]", nT, rtx_srf_moments_max_temps());
  if (nE < 1) RTX_FAIL("nE=%lld: need at least 1 emissivity column", (long long)nE);
  if (srfv_check_bands(grid, nB, knot_start_h)) return 1;
  if (!G_tau && !G_La && !G_Ld && !dTs && !dE) RTX_FAIL("no output: G_tau, G_La, G_Ld, dTs and dE are all NULL");
  if (!tau || !La || !Ld || !Ts_h || !Xk || !knot_start_h || !knot_x_d || !knot_r_d || !E || !g) RTX_FAIL("a required pointer is NULL");
  for (int t = 0; t < nT; ++t)
    if (!(Ts_h[t] > 0.0)) RTX_FAIL("surface temperature %g", Ts_h[t]);
  const long long neb = ((long long)nE + 255) / 256;
  if (neb > 65535) RTX_FAIL("nE=%lld: too many columns for one call", (long long)nE);
  if (((long long)nk * nT + 255) / 256 > 65535) RTX_FAIL("nk=%lld x nT=%d: too many for one call", (long long)nk, nT);
  hipStream_t st = (hipStream_t)stream;
  const long long nx = grid->n, n_chunks = (nx + SRF_CH - 1) / SRF_CH;
  if (nB == 0) {  // no band: the gradient of nothing
    if (G_tau) RTX_HIP(hipMemsetAsync(G_tau, 0, (size_t)nx * sizeof(float), st));
    if (G_La) RTX_HIP(hipMemsetAsync(G_La, 0, (size_t)nx * sizeof(float), st));
    if (G_Ld) RTX_HIP(hipMemsetAsync(G_Ld, 0, (size_t)nx * sizeof(float), st));
    if (dTs) RTX_HIP(hipMemsetAsync(dTs, 0, (size_t)nT * sizeof(double), st));
    if (dE) RTX_HIP(hipMemsetAsync(dE, 0, (size_t)nk * (size_t)nE * sizeof(double), st));
    return 0;
  }
  const bool rows = G_tau || G_La || G_Ld || dTs;
  const size_t nM = (size_t)nT * (size_t)nB * (size_t)nk;
  SrfvCarve c;
  const size_t o_sup = c.take((size_t)nB * 2 * sizeof(long long)), o_jr = c.take((size_t)nB * sizeof(int2)),
               o_ks = c.take(((size_t)nB + 1) * sizeof(int)), o_wn = c.take((size_t)n_chunks * nB * sizeof(double)),
               o_n = c.take((size_t)nB * sizeof(float)), o_inv = c.take((size_t)nB * sizeof(double)),
               o_sg = c.take((size_t)nB * sizeof(double)), o_part = c.take((size_t)(n_chunks > 0 ? n_chunks : 1) * nT * sizeof(double)),
               o_h = c.take(rows ? nM * sizeof(float) : 0), o_m = c.take(dE ? nM * sizeof(float) : 0),
               o_mn = c.take(dE ? (size_t)nB * sizeof(float) : 0), o_mc = c.take(dE ? (size_t)nB * sizeof(float) : 0),
               o_mj = c.take(dE ? (size_t)nB * sizeof(int2) : 0);
  char* base = nullptr;
  if (srfv_scratch->get(st, c.off, (void**)&base)) return 1;
  SrfvArgs a;
  srfv_base(a, grid, knot_x_d, knot_r_d, nB);
  a.tau = tau; a.La = La; a.Ld = Ld; a.E = E; a.g = g; a.Xk = Xk; a.nk = nk; a.nE = nE; a.nT = nT;
  for (int t = 0; t < SRFV_MAXT; ++t) a.ct[t] = t < nT ? c2l2e_over(Ts_h[t]) : 0.0;
  a.sup = (long long*)(base + o_sup); a.jr = (int2*)(base + o_jr); a.ksd = (int*)(base + o_ks); a.WN = (double*)(base + o_wn);
  a.N = (float*)(base + o_n); a.invN = (double*)(base + o_inv); a.SgT = (double*)(base + o_sg); a.part = (double*)(base + o_part);
  a.H = (float*)(base + o_h); a.M = (const float*)(base + o_m);
  a.Gt = G_tau; a.Ga = G_La; a.Gd = G_Ld; a.dTs = dTs; a.dE = dE;
  if (dE) {  // M as the forward forms it; its N equals ours bit for bit
    if (rtx_srf_moments(grid, tau, La, Ld, Ts_h, nT, Xk, nk, nB, knot_start_h, knot_x_d, knot_r_d, (float*)(base + o_mn),
                        (float*)(base + o_mc), (float*)(base + o_m), (int32_t*)(base + o_mj), stream))
      return 1;
  }
  if (srfv_norms(a, knot_start_h, n_chunks, st)) return 1;
  if (rows) {
    hipLaunchKernelGGL(srfv_h_kernel, dim3((unsigned)nB), dim3(256), 0, st, a);
    RTX_LAUNCH_CHECK();
    if (n_chunks > 0) {
      hipLaunchKernelGGL(srfv_point_kernel, dim3((unsigned)n_chunks), dim3(SRF_CH), 0, st, a);
      RTX_LAUNCH_CHECK();
    }
    if (dTs) {
      hipLaunchKernelGGL(srfv_dts_kernel, dim3(1), dim3(64), 0, st, a, n_chunks);
      RTX_LAUNCH_CHECK();
    }
  }
  if (dE) {
    hipLaunchKernelGGL(srfv_de_kernel, dim3((unsigned)nk, (unsigned)neb), dim3(256), 0, st, a);
    RTX_LAUNCH_CHECK();
  }
  return 0;
}
