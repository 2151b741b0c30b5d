// Per-pixel HSI cube for any sensor (include/radtxfr_hip.h, rtx_srf_pixel_cube): every pixel has its own
// emissivity mixture and its own surface temperature T_p, the bands are response tables of any width. The Planck function
// is interpolated IN TEMPERATURE through Q nodes T_q of the scene's range [T_lo, T_hi]:
//
//   G[e][q][b] = sum_{j in jrange[b]} M[q][b][j] E[j][e]                                  (rtx_srf_cube_tables)
//   l_q(T)     = prod_{r != q} (T - T_r) / prod_{r != q} (T_q - T_r)
//   cube[b][p] = ( C_b + sum_m frac[p][m] sum_q l_q(T_p) G[kidx[p][m]][q][b] ) / N_b      (rtx_srf_pixel_cube)
//
// with N, C, M[q] = rtx_srf_moments at the node temperatures, used unchanged: those evaluate Planck at every grid point, so
// nothing here depends on a band being narrow (rtx_pixel_cube interpolates in wavenumber across a band and does). The Ld
// term inside M rides through exactly because sum_q l_q = 1. No Planck function, no transcendental in this file.
//
// Pixel kernel, after pixel_cube_kernel (rtx_radiance.hip): lane = band, a workgroup of 256 threads owns SC_PB = 256 pixels
// x 64 bands, a wave walks 16 pixels of every round of 64, SC_PU = 4 side by side (two with the table in global memory;
// independent chains: the kernel waits on latency, not on throughput); N_b and C_b sit in the lane's registers; the values
// leave through a 64 x 65 LDS tile so that the cube is written in 256-byte rows along the pixel axis.
//   weights   thread t of the workgroup forms l_q(T) of pixel t, ONCE per pixel: numerator and denominator are fp64
//             products over r ascending (the denominators on the host, in the same order), one fp64 division, one rounding
//             to fp32, parked in LDS. A pixel exactly at node q has numerator = denominator bit for bit, so weight 1, and a
//             zero factor in every other numerator, so weight 0. A temperature that is NaN or outside [T_lo, T_hi] gets NaN
//             weights: its whole column is NaN (no extrapolation, no device-to-host check).
//   mixtures  the kidx / frac of a round's 64 pixels are staged in LDS SC_MIXC = 4 endmembers at a time (coalesced reads, the
//             indices clamped to [0, nEnd) there); a mixture of more than 4 carries its partial sum through the tile.
//   table     the [nEnd][Q][64 bands] slice of tab is staged in LDS when nEnd * Q <= SC_TAB_LDS (128: 32 KiB beside the
//             26 KiB of tile, weights and mixtures, inside the 64 KiB every launch may ask for), four nodes to a 16-byte
//             read; otherwise it is read from global memory with consecutive lanes on consecutive words (L1 / L2).
// Arithmetic of one value, the same wherever the table lies:
//   s = 0;  for m ascending { t = 0;  for q ascending t = fmaf(l_q, G[k_m][q][b], t);  s = fmaf(frac_m, t, s); }
//   cube = (C_b + s) / N_b          (all fp32; N_b = 0 gives 0 / 0 = NaN: the dead band of every srf path)
// Determinism: cube[b][p] is a pure function of (pixel p's kidx, frac and T; band b's N, C and tab column; the nodes and
// the range). Same bits run to run, for any nPix, any position of the pixel in the scene, any subset of the bands (order
// kept), and for the table in LDS or in global memory. No atomics.
#include "rtx_common.h"

#define SC_QMAX 8       // nodes: rtx_srf_moments takes 8 temperatures per call, so one call serves
#define SC_PB 256       // pixels per workgroup
#define SC_MIXC 4       // endmembers of a mixture staged at a time (8: 2 KiB more LDS, one workgroup per CU fewer at C5, 48.7 -> 42.3 us)
#define SC_TAB_LDS 128  // nEnd * Q up to which the table slice lives in LDS (x 256 bytes)
#define SC_PU 4         // pixels a wave carries side by side: a divisor of 16 with SC_PU * max(SC_QMAX, SC_MIXC) <= 64 lanes

// ---- tables: one fp32 fmaf chain per entry over the knots of jrange[b] ascending; lane = endmember (band_mix_stacked_kernel)
struct SrfCubeTabArgs {
  const float* M;  // [Q][nB][nk]
  const int2* jrange;
  int nB, Q;
  long long nk, nEnd;
  const float* E;  // [nk][nEnd]
  float* tab;      // [nEnd][Q][nB]
};

__global__ __launch_bounds__(64) void srf_cube_tables_kernel(SrfCubeTabArgs a) {
  const int b = blockIdx.x;
  const long long k = (long long)blockIdx.y * 64 + threadIdx.x;
  if (k >= a.nEnd) return;
  const int2 jr = a.jrange[b];
  float acc[SC_QMAX];
#pragma unroll
  for (int q = 0; q < SC_QMAX; ++q) acc[q] = 0.f;
#pragma unroll 4  // the loads of four knots in flight; each chain still takes its knots in ascending order
  for (int j = jr.x; j <= jr.y; ++j) {
    const float e = a.E[(size_t)j * a.nEnd + k];
#pragma unroll
    for (int q = 0; q < SC_QMAX; ++q)
      if (q < a.Q) acc[q] = fmaf(a.M[((size_t)q * a.nB + b) * a.nk + j], e, acc[q]);
  }
#pragma unroll
  for (int q = 0; q < SC_QMAX; ++q)
    if (q < a.Q) a.tab[((size_t)k * a.Q + q) * a.nB + b] = acc[q];
}

extern "C" int rtx_srf_cube_max_nodes(void) { return SC_QMAX; }

extern "C" int rtx_srf_cube_tables(const float* M, const int32_t* jrange, int nB, int Q, int64_t nk, const float* E, int64_t nEnd,
                                   float* tab, void* stream) {
  if (Q < 1 || Q > SC_QMAX) RTX_FAIL("Q=%d outside [1,%d]", Q, SC_QMAX);
  if (nB < 0 || nEnd < 0) RTX_FAIL("negative size");
  if (nk < 1) RTX_FAIL("nk=%lld: need at least 1 emissivity knot", (long long)nk);
  if (nB == 0 || nEnd == 0) return 0;
  if (!M || !jrange || !E || !tab) RTX_FAIL("a required pointer is NULL");
  const long long neb = (nEnd + 63) / 64;
  if (neb > 65535) RTX_FAIL("nEnd=%lld: too many endmembers for one call", (long long)nEnd);
  SrfCubeTabArgs a;
  a.M = M; a.jrange = reinterpret_cast<const int2*>(jrange); a.nB = nB; a.Q = Q; a.nk = nk; a.nEnd = nEnd; a.E = E; a.tab = tab;
  hipLaunchKernelGGL(srf_cube_tables_kernel, dim3((unsigned)nB, (unsigned)neb), dim3(64), 0, (hipStream_t)stream, a);
  RTX_LAUNCH_CHECK();
  return 0;
}

// ---- pixels
struct SrfCubeArgs {
  int nB, nEnd, nMix;
  long long nPix;
  double Tn[SC_QMAX];   // the nodes
  double den[SC_QMAX];  // prod_{r != q} (T_q - T_r), r ascending
  double T_lo, T_hi;
  const float *N, *C;
  const float* tab;    // [nEnd][Q][nB]
  const int* kidx;     // [nPix][nMix]
  const float* frac;   // [nPix][nMix]
  const double* Tpix;  // [nPix]
  float* cube;         // [nB][nPix]
};

// Row k of the table for this lane's band. LDS layout of an endmember's Q x 64 words: the nodes in fours, [Q / 4][64 lanes][4],
// then the Q % 4 left over as [Q % 4][64 lanes]: a lane reads four nodes in one 16-byte access, 64 lanes 1 KiB without a conflict.
template <int Q, bool TAB_LDS>
__device__ __forceinline__ void sc_row(float (&G)[Q], const float* tab, int k, int lane, size_t nB) {
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

template <int Q, bool TAB_LDS>
__global__ __launch_bounds__(256) void srf_pixel_cube_kernel(SrfCubeArgs a) {
  extern __shared__ float4 s_dyn[];  // TAB_LDS: [nEnd][Q x 64] in sc_row's layout
  __shared__ float s_tile[64][65];
  __shared__ __attribute__((aligned(16))) float s_w[SC_PB][Q];
  __shared__ int s_k[64 * SC_MIXC];
  __shared__ float s_f[64 * SC_MIXC];
  float* s_tab = reinterpret_cast<float*>(s_dyn);
  constexpr int PU = TAB_LDS ? SC_PU : SC_PU / 2;  // table in global memory: four pixels' 64-bit row addresses spilled scalar registers
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b0 = blockIdx.y * 64;
  const int b = min(b0 + lane, a.nB - 1);
  const long long p0 = (long long)blockIdx.x * SC_PB;
  const int n_pl = (int)min((long long)SC_PB, a.nPix - p0);  // pixels of this workgroup (>= 1)
  const int nMix = a.nMix, k_max = a.nEnd - 1;
  {  // the weights of pixel threadIdx.x (past the end: the last pixel's again, never used for a store)
    const double T = a.Tpix[p0 + min((int)threadIdx.x, n_pl - 1)];
    const bool ok = T >= a.T_lo && T <= a.T_hi;  // false for NaN
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      double num = 1.0;
#pragma unroll
      for (int r = 0; r < Q; ++r)
        if (r != q) num *= T - a.Tn[r];
      s_w[threadIdx.x][q] = ok ? (float)(num / a.den[q]) : __builtin_nanf("");
    }
  }
  if (TAB_LDS) {
    const int n = a.nEnd * Q * 64;
    for (int i = threadIdx.x; i < n; i += 256) {
      const int k = i / (Q * 64), rem = i - k * (Q * 64), q = rem >> 6, l = rem & 63;
      const int at = q < 4 * (Q / 4) ? ((q >> 2) * 64 + l) * 4 + (q & 3) : (Q / 4) * 256 + (q - 4 * (Q / 4)) * 64 + l;
      s_tab[k * (Q * 64) + at] = a.tab[((size_t)k * Q + q) * a.nB + min(b0 + l, a.nB - 1)];
    }
  }
  const float Cb = a.C[b], Nb = a.N[b];
  const float* tab = TAB_LDS ? s_tab : a.tab + b;
  for (int g = 0; g < SC_PB / 64; ++g) {
    if (g * 64 >= n_pl) break;  // uniform over the workgroup
    for (int m0 = 0; m0 < nMix; m0 += SC_MIXC) {
      const int mc = min(SC_MIXC, nMix - m0);
      __syncthreads();  // the weights and the table are written (first pass); the last pass' mixtures and tile are read
      for (int e = threadIdx.x; e < 64 * mc; e += 256) {
        const int pl = e / mc, m = e - pl * mc;
        const long long at = (p0 + min(g * 64 + pl, n_pl - 1)) * nMix + m0 + m;
        s_k[pl * SC_MIXC + m] = min(max(a.kidx[at], 0), k_max);  // an index outside the table must not leave it
        s_f[pl * SC_MIXC + m] = a.frac[at];
      }
      __syncthreads();
      for (int i = 0; i < 16; i += PU) {  // PU pixels side by side: their chains are independent, each one's order is as written
        const int pl = wave * 16 + i;
        // what the group's pixels own is wave-uniform: it is read from LDS once into the lanes, one (pixel, node) and one
        // (pixel, endmember slot) per lane, and taken out of them with v_readlane (pixel_cube_kernel's staging)
        const int wl = min(lane, PU * Q - 1), ml = min(lane, PU * SC_MIXC - 1);
        const float wv = s_w[min(g * 64 + pl + wl / Q, n_pl - 1)][wl % Q];  // past the end: the last pixel again, not written
        const int kv = s_k[pl * SC_MIXC + ml];
        const float fv = s_f[pl * SC_MIXC + ml];
        float w[PU][Q], s[PU];
#pragma unroll
        for (int u = 0; u < PU; ++u) {
#pragma unroll
          for (int q = 0; q < Q; ++q) w[u][q] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wv), u * Q + q));
          s[u] = m0 == 0 ? 0.f : s_tile[lane][pl + u];
        }
        for (int m = 0; m < mc; ++m) {
#pragma unroll
          for (int u = 0; u < PU; ++u) {
            const int k = __builtin_amdgcn_readlane(kv, u * SC_MIXC + m);
            const float fr = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(fv), u * SC_MIXC + m));
            float G[Q];
            sc_row<Q, TAB_LDS>(G, tab, k, lane, (size_t)a.nB);
            float t = 0.f;
#pragma unroll
            for (int q = 0; q < Q; ++q) t = fmaf(w[u][q], G[q], t);
            s[u] = fmaf(fr, t, s[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < PU; ++u) s_tile[lane][pl + u] = m0 + mc == nMix ? (Cb + s[u]) / Nb : s[u];
      }
    }
    __syncthreads();
    if (g * 64 + lane < n_pl) {
      float* dst = a.cube + (size_t)b0 * a.nPix + p0 + g * 64 + lane;
#pragma unroll 4
      for (int r = wave * 16; r < wave * 16 + 16; ++r)
        if (b0 + r < a.nB) dst[(size_t)r * a.nPix] = s_tile[r][lane];
    }
  }
}

template <int Q>
static void launch_srf_pixel_cube(const SrfCubeArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)((a.nPix + SC_PB - 1) / SC_PB), (unsigned)((a.nB + 63) / 64));
  if ((long long)a.nEnd * Q <= SC_TAB_LDS)
    hipLaunchKernelGGL((srf_pixel_cube_kernel<Q, true>), grid, dim3(256), (size_t)a.nEnd * Q * 64 * sizeof(float), stream, a);
  else
    hipLaunchKernelGGL((srf_pixel_cube_kernel<Q, false>), grid, dim3(256), 0, stream, a);
}

extern "C" int rtx_srf_pixel_cube(int nB, int Q, const double* T_node_h, const float* N, const float* C, const float* tab, int nEnd,
                                  int64_t nPix, int nMix, const int32_t* kidx, const float* frac, const double* Tpix, float* cube,
                                  void* stream) {
  if (Q < 1 || Q > SC_QMAX) RTX_FAIL("Q=%d outside [1,%d]", Q, SC_QMAX);
  if (nB < 0 || nPix < 0) RTX_FAIL("negative size");
  if (nEnd < 1 || nMix < 1) RTX_FAIL("nEnd=%d, nMix=%d: need at least 1 of each", nEnd, nMix);
  if (!T_node_h) RTX_FAIL("a required pointer is NULL");
  SrfCubeArgs a;
  a.T_lo = T_node_h[Q]; a.T_hi = T_node_h[Q + 1];
  if (!(a.T_lo > 0.0) || !isfinite(a.T_hi) || !(a.T_lo <= a.T_hi)) RTX_FAIL("temperature range [%g, %g]", a.T_lo, a.T_hi);
  for (int q = 0; q < SC_QMAX; ++q) { a.Tn[q] = 0.0; a.den[q] = 1.0; }
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
  if (nB == 0 || nPix == 0) return 0;
  if (!N || !C || !tab || !kidx || !frac || !Tpix || !cube) RTX_FAIL("a required pointer is NULL");
  if ((nPix + SC_PB - 1) / SC_PB > 0x7fffffffLL) RTX_FAIL("nPix=%lld: too many pixels for one call", (long long)nPix);
  if ((nB + 63) / 64 > 65535) RTX_FAIL("nB=%d: too many bands for one call", nB);
  a.nB = nB; a.nEnd = nEnd; a.nMix = nMix; a.nPix = nPix;
  a.N = N; a.C = C; a.tab = tab; a.kidx = kidx; a.frac = frac; a.Tpix = Tpix; a.cube = cube;
  hipStream_t st = (hipStream_t)stream;
  switch (Q) {
    case 1: launch_srf_pixel_cube<1>(a, st); break;
    case 2: launch_srf_pixel_cube<2>(a, st); break;
    case 3: launch_srf_pixel_cube<3>(a, st); break;
    case 4: launch_srf_pixel_cube<4>(a, st); break;
    case 5: launch_srf_pixel_cube<5>(a, st); break;
    case 6: launch_srf_pixel_cube<6>(a, st); break;
    case 7: launch_srf_pixel_cube<7>(a, st); break;
    default: launch_srf_pixel_cube<8>(a, st); break;
  }
  RTX_LAUNCH_CHECK();
  return 0;
}
