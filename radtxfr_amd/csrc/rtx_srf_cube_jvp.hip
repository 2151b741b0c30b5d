// Tangent of the per-pixel HSI cube under response tables (include/radtxfr_hip.h, rtx_srf_pixel_cube_jvp):
// J v of rtx_srf_pixel_cube, the exact transpose of rtx_srf_pixel_cube_vjp. With N, G = tab, l_q and l'_q as there and
// L[q][b][e] = (C_b + G[e][q][b]) / N_b the band radiance of pure endmember e at node q (column nEnd: the surface of emissivity
// 0), a direction (d_frac, d_Tpix, dL) moves the cube by
//   t_m  = sum_q l_q(T_p)  G[k_pm][q][b],   t'_m = sum_q l'_q(T_p) G[k_pm][q][b],   s_m = sum_q l_q(T_p) dL[v][q][b][k_pm]
//   d_cube[v][b][p] = sum_m ( d_frac[v][p][m] t_m + d_Tpix[v][p] frac[p][m] t'_m ) / N_b
//                   + sum_m frac[p][m] s_m + (1 - sum_m frac[p][m]) dL[v][0][b][nEnd]
// dL is what rtx_srf_radiance_jvp writes at Ts = the nodes, E' = [E | 0].
//
// Three kernels, no atomics:
//   scj_weight_kernel  one thread per pixel: l_q(T_p) and l'_q(T_p), fp64 to one fp32 rounding, into the workspace
//                      (scv_weight_kernel's code: srf_cube_weight of rtx_srf_cube_common.h).
//   scj_relay_kernel   dL [n_vec][Q][nB][nEnd + 1] -> the workspace [n_vec][nEnd + 1][Q][nB], bands innermost, through a
//                      64 x 65 LDS tile: the pixel kernel then reads 256-byte rows, as it reads the table.
//   scj_pixel_kernel   after srf_pixel_cube_kernel / scv_pixel_kernel: lane = band, a workgroup of 256 threads owns 256 pixels x
//                      64 bands in rounds of 64 pixels, a wave walks 16 pixels of every round; the table slice in LDS when
//                      nEnd * Q <= SCJ_TAB_LDS, else read from global memory. A pixel's weights and its mixture (kidx, frac,
//                      d_frac of every vector, up to 64 slots at a time) are read once into the lanes and taken out of them
//                      with v_readlane: no staging in LDS, no barrier inside a round, and the fp64 sums of a mixture of any
//                      length stay in registers. The vectors of a launch share the weights, the mixture, the table rows and
//                      t_m, t'_m; each adds its own chain s_m over its dL rows (global memory, L1 / L2: a slice is the size of
//                      the table, and LDS has no room for one per vector). d_cube leaves through one 64 x 64 LDS tile per
//                      vector, column index xor band (conflict-free both ways, 16 KiB against the 64 x 65 tile's 16.25),
//                      in 256-byte rows along the pixel axis.
// LDS: the table slice, at most 32 KiB, and SCJ_NV = 2 tiles of 16 KiB: 64 KiB, the most a workgroup of this library asks
// for. That is what sets rtx_srf_pixel_cube_jvp_max_vectors() = 2.
// Arithmetic of one value, the same wherever the table lies and whatever else the launch carries:
//   fp32, q ascending: t = fmaf(l_q, G, t), t' = fmaf(l'_q, G, t'), s = fmaf(l_q, dL, s)    (t, t' have the adjoint's bits)
//   fp64, m ascending: A = fma(d_frac, t, A); A = fma(d_Tpix * frac, t', A); B = fma(frac, s, B); F = F + frac
//   d_cube = (float)fma(1 - F, dL[v][0][b][nEnd], A / (double)N_b + B)
// An absent group enters as +0.0 and its loads and chain are skipped: the bits of zeros passed. A dead band (N_b = 0) and a
// pixel that is not admitted are NaN by a select at the store.
// Determinism: d_cube[v][b][p] is a pure function of (pixel p's kidx, frac, T and tangents; band b's N and table column;
// vector v's dL column; the nodes and the range): the same bits run to run, for any nPix, any position of the pixel, any subset
// of the bands (order kept), for a vector alone or beside another, and for the table in LDS or in global memory.
#include "rtx_common.h"
#include "rtx_srf_cube_common.h"

#define SCJ_QMAX 8       // rtx_srf_cube_max_nodes()
#define SCJ_PB 256       // pixels per workgroup of the pixel kernel
#define SCJ_TAB_LDS 128  // nEnd * Q up to which the pixel kernel holds the table slice in LDS (rtx_srf_cube.hip's SC_TAB_LDS)
#define SCJ_NV 2         // vectors per call: one 16 KiB output tile each beside 32 KiB of table

struct ScjArgs {
  int nB, nEnd, nMix, n_vec;
  long long nPix;
  double Tn[SCJ_QMAX];   // the nodes
  double den[SCJ_QMAX];  // prod_{r != q} (T_q - T_r), r ascending
  double T_lo, T_hi;
  const float* N;
  const float* tab;      // [nEnd][Q][nB]
  const int* kidx;       // [nPix][nMix]
  const float* frac;     // [nPix][nMix]
  const double* Tpix;    // [nPix]
  const float* d_frac;   // [n_vec][nPix][nMix] or NULL
  const double* d_Tpix;  // [n_vec][nPix] or NULL
  const float* dL;       // [n_vec][Q][nB][nEnd + 1] or NULL
  float* dLr;            // workspace [n_vec][nEnd + 1][Q][nB]; NULL with dL
  float* W;              // workspace [nPix][2 Q]: l_q(T_p), then l'_q(T_p); zeros for a pixel that is not admitted
  float* d_cube;         // [n_vec][nB][nPix]
};

// one thread per pixel: scv_weight_kernel's values
template <int Q>
__global__ __launch_bounds__(256) void scj_weight_kernel(ScjArgs a) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.nPix) return;
  const double T = a.Tpix[p];
  const bool ok = T >= a.T_lo && T <= a.T_hi;  // false for NaN
  float* w = a.W + (size_t)p * (2 * Q);
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    double l, dl;
    srf_cube_weight<Q>(a, T, q, l, dl);
    w[q] = ok ? (float)l : 0.f;  // the pixel kernel makes the column of a pixel that is not admitted NaN
    w[Q + q] = ok ? (float)dl : 0.f;
  }
}

// blockIdx.z = (vector, node); a tile of 64 bands x 64 columns of dL, read along the columns, written along the bands
__global__ __launch_bounds__(256) void scj_relay_kernel(ScjArgs a, int Q) {
  __shared__ float s_tile[64][65];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int e0 = blockIdx.x * 64, b0 = blockIdx.y * 64;
  const int v = blockIdx.z / Q, q = blockIdx.z - v * Q;
  const int nC = a.nEnd + 1;
  const float* src = a.dL + ((size_t)v * Q + q) * (size_t)a.nB * (size_t)nC;
  for (int r = wave * 16; r < wave * 16 + 16; ++r)
    if (b0 + r < a.nB && e0 + lane < nC) s_tile[r][lane] = src[(size_t)(b0 + r) * nC + e0 + lane];
  __syncthreads();
  for (int r = wave * 16; r < wave * 16 + 16; ++r)
    if (e0 + r < nC && b0 + lane < a.nB)
      a.dLr[(((size_t)v * nC + (size_t)(e0 + r)) * Q + q) * (size_t)a.nB + b0 + lane] = s_tile[lane][r];
}

// Row k of the table for this lane's band: sc_row of rtx_srf_cube.hip, the same LDS layout.
template <int Q, bool TAB_LDS>
__device__ __forceinline__ void scj_row(float (&G)[Q], const float* tab, int k, int lane, size_t nB) {
  if (TAB_LDS) {
    const float* base = tab + k * (Q * 64);
#pragma unroll
    for (int v = 0; v < Q / 4; ++v) {
      const float4 x = reinterpret_cast<const float4*>(base)[v * 64 + lane];
      G[4 * v] = x.x; G[4 * v + 1] = x.y; G[4 * v + 2] = x.z; G[4 * v + 3] = x.w;
    }
#pragma unroll
    for (int q = 4 * (Q / 4); q < Q; ++q) G[q] = base[(Q / 4) * 256 + (q - 4 * (Q / 4)) * 64 + lane];
  } else {
    const float* row = tab + (size_t)k * Q * nB;  // tab already points at this lane's band
#pragma unroll
    for (int q = 0; q < Q; ++q) G[q] = row[(size_t)q * nB];
  }
}

__device__ __forceinline__ float scj_lane(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

template <int Q, bool TAB_LDS, int NV>
__global__ __launch_bounds__(256) void scj_pixel_kernel(ScjArgs a) {
  extern __shared__ float4 s_dyn[];  // TAB_LDS: [nEnd][Q x 64] in scj_row's layout
  __shared__ float s_tile[NV][64][64];  // [vector][band][pixel of the round ^ band]
  float* s_tab = reinterpret_cast<float*>(s_dyn);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b0 = blockIdx.y * 64;
  const int b = min(b0 + lane, a.nB - 1);
  const long long p0 = (long long)blockIdx.x * SCJ_PB;
  const int n_pl = (int)min((long long)SCJ_PB, a.nPix - p0);  // pixels of this workgroup (>= 1)
  const int nMix = a.nMix, k_max = a.nEnd - 1;
  const size_t nB = (size_t)a.nB;
  if (TAB_LDS) {
    const int n = a.nEnd * Q * 64;
    for (int i = threadIdx.x; i < n; i += 256) {
      const int k = i / (Q * 64), rem = i - k * (Q * 64), q = rem >> 6, l = rem & 63;
      const int at = q < 4 * (Q / 4) ? ((q >> 2) * 64 + l) * 4 + (q & 3) : (Q / 4) * 256 + (q - 4 * (Q / 4)) * 64 + l;
      s_tab[k * (Q * 64) + at] = a.tab[((size_t)k * Q + q) * nB + min(b0 + l, a.nB - 1)];
    }
  }
  const float Nb = a.N[b];
  const bool live = Nb > 0.f;
  const double Nd = (double)Nb;
  const float* tab = TAB_LDS ? s_tab : a.tab + b;
  const bool has_dl = a.dLr != nullptr, has_df = a.d_frac != nullptr, has_dt = a.d_Tpix != nullptr;  // uniform
  const size_t v_stride = (size_t)(a.nEnd + 1) * Q * nB;  // one vector's slice of dLr
  const float* dlr = has_dl ? a.dLr + b : nullptr;
  double dL0[NV];  // the tangent of the bare surface's radiance, taken at node 0 as the adjoint places its cotangent
#pragma unroll
  for (int v = 0; v < NV; ++v) dL0[v] = has_dl ? (double)dlr[v * v_stride + (size_t)a.nEnd * Q * nB] : 0.0;
  for (int g = 0; g < SCJ_PB / 64; ++g) {
    if (g * 64 >= n_pl) break;  // uniform over the workgroup
    __syncthreads();            // the table is written (first round); the last round's tiles are read
    for (int i = 0; i < 16; ++i) {
      const int pl = wave * 16 + i;
      if (g * 64 + pl >= n_pl) break;  // uniform over the wave: what the tile holds there is never stored
      const long long p = p0 + g * 64 + pl;
      const double T = a.Tpix[p];
      const bool okp = T >= a.T_lo && T <= a.T_hi;  // false for NaN
      float w[Q], wp[Q];
      {
        const float wv = a.W[(size_t)p * (2 * Q) + min(lane, 2 * Q - 1)];
#pragma unroll
        for (int q = 0; q < Q; ++q) { w[q] = scj_lane(wv, q); wp[q] = scj_lane(wv, Q + q); }
      }
      double dTv[NV], A[NV], B[NV], F = 0.0;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        dTv[v] = has_dt ? a.d_Tpix[(size_t)v * (size_t)a.nPix + (size_t)p] : 0.0;
        A[v] = 0.0; B[v] = 0.0;
      }
      for (int m0 = 0; m0 < nMix; m0 += 64) {
        const int mc = min(64, nMix - m0);
        const size_t at = (size_t)p * nMix + m0 + min(lane, mc - 1);  // lane = slot (past the end: the last slot again, not used)
        const int kv = min(max(a.kidx[at], 0), k_max);                // clamped as the forward clamps it
        const float fv = a.frac[at];
        float dfv[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) dfv[v] = has_df ? a.d_frac[(size_t)v * (size_t)a.nPix * nMix + at] : 0.f;
        for (int m = 0; m < mc; ++m) {
          const int k = __builtin_amdgcn_readlane(kv, m);
          const float fr = scj_lane(fv, m);
          float G[Q];
          scj_row<Q, TAB_LDS>(G, tab, k, lane, nB);
          float t = 0.f, tp = 0.f;
#pragma unroll
          for (int q = 0; q < Q; ++q) { t = fmaf(w[q], G[q], t); tp = fmaf(wp[q], G[q], tp); }
          F += (double)fr;
#pragma unroll
          for (int v = 0; v < NV; ++v) {
            float s = 0.f;
            if (has_dl) {
              const float* row = dlr + v * v_stride + (size_t)k * Q * nB;
#pragma unroll
              for (int q = 0; q < Q; ++q) s = fmaf(w[q], row[(size_t)q * nB], s);
            }
            A[v] = fma((double)scj_lane(dfv[v], m), (double)t, A[v]);
            A[v] = fma(dTv[v] * (double)fr, (double)tp, A[v]);
            B[v] = fma((double)fr, (double)s, B[v]);
          }
        }
      }
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const double r = fma(1.0 - F, dL0[v], A[v] / Nd + B[v]);
        s_tile[v][lane][(pl ^ lane) & 63] = (live && okp) ? (float)r : __builtin_nanf("");  // a select, not 0 * inf
      }
    }
    __syncthreads();
    if (g * 64 + lane < n_pl) {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        float* dst = a.d_cube + ((size_t)v * nB + (size_t)b0) * (size_t)a.nPix + (size_t)p0 + g * 64 + lane;
#pragma unroll 4
        for (int r = wave * 16; r < wave * 16 + 16; ++r)
          if (b0 + r < a.nB) dst[(size_t)r * (size_t)a.nPix] = s_tile[v][r][(lane ^ r) & 63];
      }
    }
  }
}

// workspace per (device, stream), as rtx_srf_pixel_cube_vjp's
static StreamScratch* const scj_scratch = new StreamScratch();

template <int Q, int NV>
static void launch_scj_pixels(const ScjArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)((a.nPix + SCJ_PB - 1) / SCJ_PB), (unsigned)((a.nB + 63) / 64));
  if ((long long)a.nEnd * Q <= SCJ_TAB_LDS)
    hipLaunchKernelGGL((scj_pixel_kernel<Q, true, NV>), grid, dim3(256), (size_t)a.nEnd * Q * 64 * sizeof(float), st, a);
  else
    hipLaunchKernelGGL((scj_pixel_kernel<Q, false, NV>), grid, dim3(256), 0, st, a);
}

template <int Q>
static void launch_scj(const ScjArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((scj_weight_kernel<Q>), dim3((unsigned)((a.nPix + 255) / 256)), dim3(256), 0, st, a);
  if (a.dL)
    hipLaunchKernelGGL(scj_relay_kernel, dim3((unsigned)((a.nEnd + 1 + 63) / 64), (unsigned)((a.nB + 63) / 64), (unsigned)(a.n_vec * Q)),
                       dim3(256), 0, st, a, Q);
  if (a.n_vec == 1) launch_scj_pixels<Q, 1>(a, st);
  else launch_scj_pixels<Q, SCJ_NV>(a, st);
}

extern "C" int rtx_srf_pixel_cube_jvp_max_vectors(void) { return SCJ_NV; }

extern "C" int rtx_srf_pixel_cube_jvp(int nB, int Q, const double* T_node_h, const float* N, const float* tab, int nEnd, int64_t nPix,
                                      int nMix, const int32_t* kidx, const float* frac, const double* Tpix, const float* d_frac,
                                      const double* d_Tpix, const float* dL, int n_vec, float* d_cube, void* stream, unsigned flags) {
  if (flags != 0) RTX_FAIL("rtx_srf_pixel_cube_jvp: flags=%u, none is defined", flags);
  if (Q < 1 || Q > SCJ_QMAX) RTX_FAIL("Q=%d outside [1,%d]", Q, SCJ_QMAX);
  if (nB < 0 || nPix < 0) RTX_FAIL("negative size");
  if (nEnd < 1 || nMix < 1) RTX_FAIL("nEnd=%d, nMix=%d: need at least 1 of each", nEnd, nMix);
  if (n_vec < 1 || n_vec > SCJ_NV) RTX_FAIL("n_vec=%d outside [1,%d] (rtx_srf_pixel_cube_jvp_max_vectors)", n_vec, SCJ_NV);
  if (!T_node_h) RTX_FAIL("a required pointer is NULL");
  ScjArgs a;
  memset(&a, 0, sizeof(a));
  a.T_lo = T_node_h[Q]; a.T_hi = T_node_h[Q + 1];
  if (!(a.T_lo > 0.0) || !isfinite(a.T_hi) || !(a.T_lo <= a.T_hi)) RTX_FAIL("temperature range [%g, %g]", a.T_lo, a.T_hi);
  for (int q = 0; q < SCJ_QMAX; ++q) { a.Tn[q] = 0.0; a.den[q] = 1.0; }
  for (int q = 0; q < Q; ++q) {
    const double T = T_node_h[q];
    if (!isfinite(T) || !(T > 0.0)) RTX_FAIL("node temperature %g", T);
    if (T < a.T_lo || T > a.T_hi) RTX_FAIL("node temperature %g outside the range [%g, %g]", T, a.T_lo, a.T_hi);
    a.Tn[q] = T;
  }
  for (int q = 0; q < Q; ++q) {
    double den = 1.0;
    for (int r = 0; r < Q; ++r)
      if (r != q) den *= a.Tn[q] - a.Tn[r];
    if (den == 0.0 || !isfinite(den)) RTX_FAIL("the node temperatures are not distinct (node %d: %g)", q, a.Tn[q]);
    a.den[q] = den;
  }
  if (!d_frac && !d_Tpix && !dL) RTX_FAIL("no tangent: d_frac, d_Tpix and dL are all NULL");
  if (nB == 0 || nPix == 0) return 0;  // the tangent of nothing
  if (!N || !tab || !kidx || !frac || !Tpix || !d_cube) RTX_FAIL("a required pointer is NULL");
  if ((nPix + SCJ_PB - 1) / SCJ_PB > 0x7fffffffLL) RTX_FAIL("nPix=%lld: too many pixels for one call", (long long)nPix);
  if ((nB + 63) / 64 > 65535) RTX_FAIL("nB=%d: too many bands for one call", nB);
  a.nB = nB; a.nEnd = nEnd; a.nMix = nMix; a.nPix = nPix; a.n_vec = n_vec;
  a.N = N; a.tab = tab; a.kidx = kidx; a.frac = frac; a.Tpix = Tpix;
  a.d_frac = d_frac; a.d_Tpix = d_Tpix; a.dL = dL; a.d_cube = d_cube;
  const size_t bytesL = dL ? (size_t)n_vec * (size_t)(nEnd + 1) * (size_t)Q * (size_t)nB * sizeof(float) : 0;
  const size_t offW = (bytesL + 15) & ~(size_t)15;
  char* base = nullptr;
  if (scj_scratch->get(stream, offW + (size_t)nPix * 2 * Q * sizeof(float), (void**)&base)) return 1;
  a.dLr = dL ? (float*)base : nullptr;
  a.W = (float*)(base + offW);
  hipStream_t st = (hipStream_t)stream;
  switch (Q) {
    case 1: launch_scj<1>(a, st); break;
    case 2: launch_scj<2>(a, st); break;
    case 3: launch_scj<3>(a, st); break;
    case 4: launch_scj<4>(a, st); break;
    case 5: launch_scj<5>(a, st); break;
    case 6: launch_scj<6>(a, st); break;
    case 7: launch_scj<7>(a, st); break;
    default: launch_scj<8>(a, st); break;
  }
  RTX_LAUNCH_CHECK();
  return 0;
}
