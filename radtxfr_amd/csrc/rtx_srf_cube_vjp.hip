// Adjoint of the per-pixel HSI cube under response tables (include/radtxfr_hip.h, rtx_srf_pixel_cube_vjp):
// the transpose of rtx_srf_pixel_cube. With N, G = tab and l_q as there, the cube is
//   cube[b][p] = sum_m f_pm sum_q l_q(T_p) L[q][b][k_pm] + (1 - sum_m f_pm) L0[b],   L[q][b][e] = (C_b + G[e][q][b]) / N_b,  L0 = C / N,
// so a cotangent g[b][p] gives, with u_bp = g[b][p] on a live band (N_b > 0) and an admitted pixel, 0 otherwise (a select),
//   dfrac[p][m] = sum_b (u_bp / N_b) sum_q l_q(T_p)  G[k_pm][q][b]
//   dT[p]       = sum_b (u_bp / N_b) sum_m f_pm sum_q l'_q(T_p) G[k_pm][q][b],   l'_q = sum_{s != q} prod_{r != q, s} (T - T_r) / den_q
//   gL[q][b][e] = sum_p u_bp l_q(T_p) sum_{m: k_pm = e} f_pm   (e < nEnd),   gL[0][b][nEnd] = sum_p u_bp (1 - sum_m f_pm)
// and gL is the cotangent rtx_srf_radiance_vjp takes at Ts = the nodes and E' = [E | 0].
//
// Five kernels, no atomics:
//   scv_weight_kernel  one thread per pixel: l_q(T_p) and l'_q(T_p), fp64 to one fp32 rounding, into the workspace: every band
//                      block, chunk and slice below reads them instead of forming them again.
//   scv_pixel_kernel   after srf_pixel_cube_kernel: lane = band, a workgroup of 256 threads owns 256 pixels x 64 bands in rounds
//                      of 64 pixels; the table slice in LDS when nEnd * Q <= SCV_TAB_LDS, else read from global memory; g comes in
//                      through a 64 x 65 LDS tile (256-byte reads along the pixel axis). A wave takes SCV_PU = 4 pixels and
//                      SCV_MIXC = 4 mixture slots side by side and sums their 16 + 4 lane values over the 64 bands with one
//                      transposing butterfly (scv_reduce): the xor tree of srfv_wave_sum, 24 cross-lane moves in place of 120.
//                      Writes the block's partial sums to the workspace, [band block][pixel][nMix + 1].
//   scv_finish_kernel  dfrac[p][m] and dT[p]: the band blocks ascending; NaN for a pixel that is not admitted.
//   scv_gl_kernel      ONE WAVE per (pixel chunk, 64-band block, table slice): lane = band, a private fp64 LDS accumulator
//                      [rows of the slice][64 lanes]; the wave walks its pixels ascending and adds u (l_q f) into the rows of the
//                      endmembers the pixel mixes. A lane touches its own column only. The pad column rides in a register of
//                      slice 0. Writes the chunk's sums to the workspace, [chunk][nEnd + 1][Q][nB].
//   scv_sum_kernel     gL[q][b][e]: the chunks ascending in fp64, rounded to fp32 at the store.
#include "rtx_common.h"
#include "rtx_srf_cube_common.h"

#define SCV_QMAX 8       // rtx_srf_cube_max_nodes()
#define SCV_PB 256       // pixels per workgroup of the pixel kernel
#define SCV_MIXC 4       // mixture slots staged at a time by the pixel kernel
#define SCV_PU 4         // pixels a wave carries side by side
#define SCV_TAB_LDS 128  // nEnd * Q up to which the pixel kernel holds the table slice in LDS (rtx_srf_cube.hip's SC_TAB_LDS)
#define SCV_ROWS 112     // table rows (endmember, node) of one slice of the reduction: 112 x 64 lanes x 8 bytes = 56 KiB of LDS
#define SCV_MIXB 8       // mixture slots staged at a time by the reduction
#define SCV_CHUNK 256    // pixels per chunk of the reduction, doubled until the chunk sums fit SCV_WS_MAX
#define SCV_WS_MAX (64ll << 20)

struct ScvArgs {
  int nB, nEnd, nMix;
  long long nPix;
  double Tn[SCV_QMAX];   // the nodes
  double den[SCV_QMAX];  // prod_{r != q} (T_q - T_r), r ascending
  double T_lo, T_hi;
  const float* N;
  const float* tab;    // [nEnd][Q][nB]
  const int* kidx;     // [nPix][nMix]
  const float* frac;   // [nPix][nMix]
  const double* Tpix;  // [nPix]
  const float* g;      // [nB][nPix]
  double* partA;       // [n band blocks][nPix][nMix + 1]: dfrac's and dT's sums over one block of 64 bands
  double* partB;       // [n chunks][nEnd + 1][Q][nB]: gL's sums over one chunk of pixels
  float* W;            // [nPix][2 Q]: l_q(T_p), then l'_q(T_p); zeros for a pixel that is not admitted
  long long chunk;     // pixels per chunk
  int eps;             // endmembers per slice
  int n_blk;
  long long n_chunks;
  double *dT, *dfrac;
  float* gL;
};

__device__ __forceinline__ float scv_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// l_q(T) and l'_q(T) in fp64, the products over r ascending as rtx_srf_pixel_cube forms them, one division each
template <int Q>
__device__ __forceinline__ void scv_weight(const ScvArgs& a, double T, int q, double& l, double& dl) {
  srf_cube_weight<Q>(a, T, q, l, dl);  // shared with the tangent (rtx_srf_cube_jvp.hip)
}

// Row k of the table for this lane's band: sc_row of rtx_srf_cube.hip, the same LDS layout.
template <int Q, bool TAB_LDS>
__device__ __forceinline__ void scv_row(float (&G)[Q], const float* tab, int k, int lane, size_t nB) {
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

// The sums over the 64 lanes of n items at once (n a power of two): on return v[0] of lane L holds the total of item L & (n - 1).
// Stage s pairs lanes L and L ^ (1 << s): the lane whose bit s is clear keeps the even item of a pair and hands over the odd
// one. Every item is summed along the xor tree of srfv_wave_sum (distance 1, 2, 4, ... 32), so the bits are that sum's.
template <int n>
__device__ __forceinline__ void scv_reduce(double (&v)[n], int lane) {
  int s = 0;
#pragma unroll
  for (int w = n; w > 1; w >>= 1, ++s) {
    const bool up = (lane >> s) & 1;
#pragma unroll
    for (int j = 0; j < w / 2; ++j) {
      const double keep = up ? v[2 * j + 1] : v[2 * j], send = up ? v[2 * j] : v[2 * j + 1];
      v[j] = keep + __shfl_xor(send, 1 << s, 64);
    }
  }
#pragma unroll
  for (int m = n; m < 64; m <<= 1) v[0] += __shfl_xor(v[0], m, 64);
}

// one thread per pixel: the weights every band block, chunk and slice of the two kernels below reads
template <int Q>
__global__ __launch_bounds__(256) void scv_weight_kernel(ScvArgs a) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.nPix) return;
  const double T = a.Tpix[p];
  const bool ok = T >= a.T_lo && T <= a.T_hi;  // false for NaN
  float* w = a.W + (size_t)p * (2 * Q);
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    double l, dl;
    scv_weight<Q>(a, T, q, l, dl);
    w[q] = ok ? (float)l : 0.f;  // a pixel that is not admitted adds zeros; the finish kernel makes its own entries NaN
    w[Q + q] = ok ? (float)dl : 0.f;
  }
}

template <int Q, bool TAB_LDS>
__global__ __launch_bounds__(256) void scv_pixel_kernel(ScvArgs a) {
  extern __shared__ float4 s_dyn[];  // TAB_LDS: [nEnd][Q x 64] in scv_row's layout
  __shared__ float s_tile[64][65];
  __shared__ float s_w[64][Q], s_wp[64][Q];
  __shared__ int s_ok[64];
  __shared__ int s_k[64 * SCV_MIXC];
  __shared__ float s_f[64 * SCV_MIXC];
  __shared__ double s_dT[64];
  float* s_tab = reinterpret_cast<float*>(s_dyn);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b0 = blockIdx.y * 64;
  const int b = min(b0 + lane, a.nB - 1);
  const long long p0 = (long long)blockIdx.x * SCV_PB;
  const int n_pl = (int)min((long long)SCV_PB, a.nPix - p0);  // pixels of this workgroup (>= 1)
  const int nMix = a.nMix, k_max = a.nEnd - 1;
  if (TAB_LDS) {
    const int n = a.nEnd * Q * 64;
    for (int i = threadIdx.x; i < n; i += 256) {
      const int k = i / (Q * 64), rem = i - k * (Q * 64), q = rem >> 6, l = rem & 63;
      const int at = q < 4 * (Q / 4) ? ((q >> 2) * 64 + l) * 4 + (q & 3) : (Q / 4) * 256 + (q - 4 * (Q / 4)) * 64 + l;
      s_tab[k * (Q * 64) + at] = a.tab[((size_t)k * Q + q) * a.nB + min(b0 + l, a.nB - 1)];
    }
  }
  const float Nb = a.N[b];
  const bool live = b0 + lane < a.nB && Nb > 0.f;
  const double invN = live ? 1.0 / (double)Nb : 0.0;
  const float* tab = TAB_LDS ? s_tab : a.tab + b;
  double* part = a.partA + ((size_t)blockIdx.y * (size_t)a.nPix + (size_t)p0) * (size_t)(nMix + 1);
  for (int g = 0; g < SCV_PB / 64; ++g) {
    if (g * 64 >= n_pl) break;  // uniform over the workgroup
    __syncthreads();            // the last round's weights, flags and tile are read
    // the weights of the round's 64 pixels (past the end: the last pixel's again, never used for a store)
    for (int i = threadIdx.x; i < 64 * 2 * Q; i += 256) {
      const int j = i / (2 * Q), r = i - j * (2 * Q);
      const float v = a.W[(size_t)(p0 + min(g * 64 + j, n_pl - 1)) * (2 * Q) + r];
      if (r < Q) s_w[j][r] = v; else s_wp[j][r - Q] = v;
    }
    if (threadIdx.x < 64) {
      const int j = threadIdx.x;
      const double T = a.Tpix[p0 + min(g * 64 + j, n_pl - 1)];
      s_ok[j] = (g * 64 + j < n_pl && T >= a.T_lo && T <= a.T_hi) ? 1 : 0;  // 0 for NaN
    }
    {  // the cotangent of 64 bands x 64 pixels, read along the pixel axis
      const int pix = g * 64 + lane;
      const float* src = a.g + (size_t)b0 * (size_t)a.nPix + (size_t)p0 + pix;
#pragma unroll 4
      for (int r = wave * 16; r < wave * 16 + 16; ++r)
        s_tile[r][lane] = (b0 + r < a.nB && pix < n_pl) ? src[(size_t)r * (size_t)a.nPix] : 0.f;
    }
    for (int m0 = 0; m0 < nMix; m0 += SCV_MIXC) {
      const int mc = min(SCV_MIXC, nMix - m0);
      __syncthreads();  // weights, flags, tile and (first pass) the table are written; the last pass' mixtures are read
      for (int e = threadIdx.x; e < 64 * mc; e += 256) {
        const int pl = e / mc, m = e - pl * mc;
        const long long at = (p0 + min(g * 64 + pl, n_pl - 1)) * nMix + m0 + m;
        s_k[pl * SCV_MIXC + m] = min(max(a.kidx[at], 0), k_max);  // clamped as the forward clamps it
        s_f[pl * SCV_MIXC + m] = a.frac[at];
      }
      __syncthreads();
      for (int i = 0; i < 16; i += SCV_PU) {
        const int pl = wave * 16 + i;
        double dv[SCV_PU * SCV_MIXC], dt[SCV_PU];
#pragma unroll
        for (int u = 0; u < SCV_PU; ++u) {
          const int pix = pl + u;
          const bool okp = __builtin_amdgcn_readfirstlane(s_ok[pix]) != 0;
          const float uv = (live && okp) ? s_tile[lane][pix] : 0.f;  // a select: what a dead band or a refused pixel holds is not used
          const double x = (double)uv * invN;
          float w[Q], wp[Q];
#pragma unroll
          for (int q = 0; q < Q; ++q) { w[q] = scv_uniform(s_w[pix][q]); wp[q] = scv_uniform(s_wp[pix][q]); }
          double sT = 0.0;
#pragma unroll
          for (int m = 0; m < SCV_MIXC; ++m) {
            double d = 0.0;
            if (m < mc) {  // uniform
              const int k = __builtin_amdgcn_readfirstlane(s_k[pix * SCV_MIXC + m]);
              const float fr = scv_uniform(s_f[pix * SCV_MIXC + m]);
              float G[Q];
              scv_row<Q, TAB_LDS>(G, tab, k, lane, (size_t)a.nB);
              float t = 0.f, tp = 0.f;
#pragma unroll
              for (int q = 0; q < Q; ++q) { t = fmaf(w[q], G[q], t); tp = fmaf(wp[q], G[q], tp); }
              d = x * (double)t;
              sT += (double)fr * (double)tp;
            }
            dv[u * SCV_MIXC + m] = d;
          }
          dt[u] = x * sT;
        }
        scv_reduce<SCV_PU * SCV_MIXC>(dv, lane);
        scv_reduce<SCV_PU>(dt, lane);
        if (lane < SCV_PU * SCV_MIXC) {
          const int pix = g * 64 + pl + lane / SCV_MIXC, m = lane % SCV_MIXC;
          if (m < mc && pix < n_pl) part[(size_t)pix * (nMix + 1) + m0 + m] = dv[0];
        }
        if (lane < SCV_PU) {  // dT: the passes of a long mixture are added in pass order, by the lane that wrote the last one
          const int pix = g * 64 + pl + lane;
          const double v = m0 == 0 ? dt[0] : s_dT[pl + lane] + dt[0];
          if (m0 + mc < nMix) s_dT[pl + lane] = v;
          else if (pix < n_pl) part[(size_t)pix * (nMix + 1) + nMix] = v;
        }
      }
    }
  }
}

// one thread per (pixel, slot): slots 0 .. nMix - 1 are dfrac's, slot nMix is dT's
__global__ __launch_bounds__(256) void scv_finish_kernel(ScvArgs a) {
  const long long n = a.nPix * (a.nMix + 1);
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long p = i / (a.nMix + 1);
  const int j = (int)(i - p * (a.nMix + 1));
  const double T = a.Tpix[p];
  double v = a.partA[i];
  for (int blk = 1; blk < a.n_blk; ++blk) v += a.partA[(size_t)blk * (size_t)n + (size_t)i];
  if (!(T >= a.T_lo && T <= a.T_hi)) v = __builtin_nan("");
  if (j < a.nMix) {
    if (a.dfrac) a.dfrac[p * a.nMix + j] = v;
  } else if (a.dT) {
    a.dT[p] = v;
  }
}

template <int Q>
__global__ __launch_bounds__(64) void scv_gl_kernel(ScvArgs a) {
  extern __shared__ double s_acc[];  // [rows][64 lanes]
  __shared__ float s_w[64][Q];
  __shared__ double s_fs[64];
  __shared__ int s_k[64 * SCV_MIXB];
  __shared__ float s_f[64 * SCV_MIXB];
  const int lane = threadIdx.x;
  const long long chunk = blockIdx.x;
  const int b0 = blockIdx.y * 64, slice = blockIdx.z;
  const int e0 = slice * a.eps, ne = min(a.eps, a.nEnd - e0), rows = ne * Q;
  const int b = min(b0 + lane, a.nB - 1);
  const bool live = b0 + lane < a.nB && a.N[b] > 0.f;
  const int nMix = a.nMix, k_max = a.nEnd - 1;
  const long long c0 = chunk * a.chunk, c1 = min(c0 + a.chunk, a.nPix);
  for (int r = 0; r < rows; ++r) s_acc[r * 64 + lane] = 0.0;  // a lane's own column: no other lane reads or writes it
  const float* gb = a.g + (size_t)b * (size_t)a.nPix;
  double pad = 0.0;
  for (long long pg = c0; pg < c1; pg += 64) {
    const int n = (int)min(64ll, c1 - pg);
    __syncthreads();  // the last group's weights and mixtures are read
    unsigned long long mask;
    {  // lane = pixel: its weights, and (slice 0) what its fractions leave to the bare surface
      const long long p = pg + min(lane, n - 1);
      const double T = a.Tpix[p];
      const bool ok = lane < n && T >= a.T_lo && T <= a.T_hi;
#pragma unroll
      for (int q = 0; q < Q; ++q) s_w[lane][q] = a.W[(size_t)p * (2 * Q) + q];
      mask = __ballot(ok);
      if (slice == 0) {
        double fs = 0.0;
        for (int m = 0; m < nMix; ++m) fs += (double)a.frac[p * nMix + m];
        s_fs[lane] = 1.0 - fs;
      }
    }
    for (int m0 = 0; m0 < nMix; m0 += SCV_MIXB) {
      const int mc = min(SCV_MIXB, nMix - m0);
      __syncthreads();
      for (int e = lane; e < 64 * mc; e += 64) {
        const int pl = e / mc, m = e - pl * mc;
        const long long at = (pg + min(pl, n - 1)) * nMix + m0 + m;
        s_k[pl * SCV_MIXB + m] = min(max(a.kidx[at], 0), k_max);
        s_f[pl * SCV_MIXB + m] = a.frac[at];
      }
      __syncthreads();
      unsigned long long todo;  // the admitted pixels that mix an endmember of this slice in this pass (slice 0, first pass: all admitted)
      {
        bool hit = slice == 0 && m0 == 0;
        for (int m = 0; m < mc; ++m) hit = hit || (unsigned)(s_k[lane * SCV_MIXB + m] - e0) < (unsigned)ne;
        todo = __ballot(hit) & mask;
      }
      for (int sub = 0; sub < 64; sub += 16) {
        if (sub >= n) break;
        if (((todo >> sub) & 0xffffull) == 0) continue;  // uniform: g is not read where no pixel needs it
        float uu[16];  // up to 16 pixels' cotangents in flight
#pragma unroll
        for (int ii = 0; ii < 16; ++ii) {
          const int i = sub + ii;
          uu[ii] = (live && ((todo >> i) & 1ull)) ? gb[pg + i] : 0.f;  // a select: nothing else is ever read
        }
#pragma unroll
        for (int ii = 0; ii < 16; ++ii) {
          const int i = sub + ii;
          if (!((todo >> i) & 1ull)) continue;  // uniform; a pixel that is not admitted adds nothing
          const double x = (double)uu[ii];
          if (slice == 0 && m0 == 0) pad += x * s_fs[i];
          for (int m = 0; m < mc; ++m) {
            const int k = __builtin_amdgcn_readfirstlane(s_k[i * SCV_MIXB + m]) - e0;
            if ((unsigned)k >= (unsigned)ne) continue;  // uniform: the endmember lies in another slice
            const double fr = (double)scv_uniform(s_f[i * SCV_MIXB + m]);
            double* row = s_acc + (size_t)k * (Q * 64) + lane;
#pragma unroll
            for (int q = 0; q < Q; ++q) row[q * 64] += x * ((double)scv_uniform(s_w[i][q]) * fr);
          }
        }
      }
    }
  }
  if (b0 + lane < a.nB) {
    double* dst = a.partB + ((size_t)chunk * (size_t)(a.nEnd + 1) + (size_t)e0) * (size_t)Q * (size_t)a.nB + b0 + lane;
    for (int r = 0; r < rows; ++r) dst[(size_t)r * (size_t)a.nB] = s_acc[r * 64 + lane];
    if (slice == 0) a.partB[((size_t)chunk * (size_t)(a.nEnd + 1) + (size_t)a.nEnd) * (size_t)Q * (size_t)a.nB + b0 + lane] = pad;
  }
}

// one thread per (endmember column e <= nEnd, node q, band b), b fastest: the chunks ascending
__global__ __launch_bounds__(256) void scv_sum_kernel(ScvArgs a, int Q) {
  const long long n = (long long)(a.nEnd + 1) * Q * a.nB;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int b = (int)(i % a.nB);
  const long long eq = i / a.nB;
  const int q = (int)(eq % Q);
  const long long e = eq / Q;
  float out = 0.f;
  if (e < a.nEnd || q == 0) {  // the pad column has a cotangent at node 0 only
    double v = a.partB[i];
    for (long long ch = 1; ch < a.n_chunks; ++ch) v += a.partB[(size_t)ch * (size_t)n + (size_t)i];
    out = (float)v;
  }
  a.gL[((size_t)q * a.nB + b) * (size_t)(a.nEnd + 1) + (size_t)e] = out;
}

// workspace per (device, stream), as rtx_srf_radiance_vjp's
static StreamScratch* const scv_scratch = new StreamScratch();

template <int Q>
static void launch_scv(const ScvArgs& a, bool pixels, bool reduce, hipStream_t st) {
  hipLaunchKernelGGL((scv_weight_kernel<Q>), dim3((unsigned)((a.nPix + 255) / 256)), dim3(256), 0, st, a);
  if (pixels) {
    const dim3 grid((unsigned)((a.nPix + SCV_PB - 1) / SCV_PB), (unsigned)a.n_blk);
    if ((long long)a.nEnd * Q <= SCV_TAB_LDS)
      hipLaunchKernelGGL((scv_pixel_kernel<Q, true>), grid, dim3(256), (size_t)a.nEnd * Q * 64 * sizeof(float), st, a);
    else
      hipLaunchKernelGGL((scv_pixel_kernel<Q, false>), grid, dim3(256), 0, st, a);
  }
  if (reduce) {
    const int n_slices = (a.nEnd + a.eps - 1) / a.eps;
    const int rows = (a.nEnd < a.eps ? a.nEnd : a.eps) * Q;
    hipLaunchKernelGGL((scv_gl_kernel<Q>), dim3((unsigned)a.n_chunks, (unsigned)a.n_blk, (unsigned)n_slices), dim3(64),
                       (size_t)rows * 64 * sizeof(double), st, a);
  }
}

extern "C" int rtx_srf_pixel_cube_vjp(int nB, int Q, const double* T_node_h, const float* N, const float* tab, int nEnd, int64_t nPix,
                                      int nMix, const int32_t* kidx, const float* frac, const double* Tpix, const float* g, double* dT,
                                      double* dfrac, float* gL, void* stream, unsigned flags) {
  if (flags != 0) RTX_FAIL("rtx_srf_pixel_cube_vjp: flags=%u, none is defined", flags);
  if (Q < 1 || Q > SCV_QMAX) RTX_FAIL("Q=%d outside [1,%d]", Q, SCV_QMAX);
  if (nB < 0 || nPix < 0) RTX_FAIL("negative size");
  if (nEnd < 1 || nMix < 1) RTX_FAIL("nEnd=%d, nMix=%d: need at least 1 of each", nEnd, nMix);
  if (!T_node_h) RTX_FAIL("a required pointer is NULL");
  ScvArgs a;
  memset(&a, 0, sizeof(a));
  a.T_lo = T_node_h[Q]; a.T_hi = T_node_h[Q + 1];
  if (!(a.T_lo > 0.0) || !isfinite(a.T_hi) || !(a.T_lo <= a.T_hi)) RTX_FAIL("temperature range [%g, %g]", a.T_lo, a.T_hi);
  for (int q = 0; q < SCV_QMAX; ++q) { a.Tn[q] = 0.0; a.den[q] = 1.0; }
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
  if (!dT && !dfrac && !gL) RTX_FAIL("no output: dT, dfrac and gL are all NULL");
  hipStream_t st = (hipStream_t)stream;
  if (nB == 0 || nPix == 0) {  // the gradient of nothing
    if (gL && nB > 0) RTX_HIP(hipMemsetAsync(gL, 0, (size_t)Q * (size_t)nB * (size_t)(nEnd + 1) * sizeof(float), st));
    if (dT && nPix > 0) RTX_HIP(hipMemsetAsync(dT, 0, (size_t)nPix * sizeof(double), st));
    if (dfrac && nPix > 0) RTX_HIP(hipMemsetAsync(dfrac, 0, (size_t)nPix * (size_t)nMix * sizeof(double), st));
    return 0;
  }
  if (!N || !tab || !kidx || !frac || !Tpix || !g) RTX_FAIL("a required pointer is NULL");
  if ((nPix + SCV_PB - 1) / SCV_PB > 0x7fffffffLL) RTX_FAIL("nPix=%lld: too many pixels for one call", (long long)nPix);
  if ((nB + 63) / 64 > 65535) RTX_FAIL("nB=%d: too many bands for one call", nB);
  a.eps = SCV_ROWS / Q;
  if ((nEnd + a.eps - 1) / a.eps > 65535) RTX_FAIL("nEnd=%d: too many endmembers for one call", nEnd);
  a.nB = nB; a.nEnd = nEnd; a.nMix = nMix; a.nPix = nPix;
  a.N = N; a.tab = tab; a.kidx = kidx; a.frac = frac; a.Tpix = Tpix; a.g = g;
  a.dT = dT; a.dfrac = dfrac; a.gL = gL;
  a.n_blk = (nB + 63) / 64;
  // the chunk of the reduction: a function of the sizes alone
  const size_t per_chunk = (size_t)(nEnd + 1) * (size_t)Q * (size_t)nB * sizeof(double);
  a.chunk = SCV_CHUNK;
  while (((nPix + a.chunk - 1) / a.chunk) > 1 && (size_t)((nPix + a.chunk - 1) / a.chunk) * per_chunk > (size_t)SCV_WS_MAX) a.chunk *= 2;
  a.n_chunks = (nPix + a.chunk - 1) / a.chunk;
  if (a.n_chunks > 0x7fffffffLL) RTX_FAIL("nPix=%lld: too many pixels for one call", (long long)nPix);
  const bool pixels = dT || dfrac, reduce = gL != nullptr;
  if (((long long)nPix * (nMix + 1) + 255) / 256 > 0x7fffffffLL) RTX_FAIL("nPix=%lld x nMix=%d: too many for one call", (long long)nPix, nMix);
  if (((long long)(nEnd + 1) * Q * nB + 255) / 256 > 0x7fffffffLL) RTX_FAIL("nEnd=%d x nB=%d: too many for one call", nEnd, nB);
  const size_t bytesA = pixels ? (size_t)a.n_blk * (size_t)nPix * (size_t)(nMix + 1) * sizeof(double) : 0;
  const size_t bytesB = reduce ? (size_t)a.n_chunks * per_chunk : 0;
  const size_t offB = (bytesA + 15) & ~(size_t)15, offW = offB + ((bytesB + 15) & ~(size_t)15);
  char* base = nullptr;
  if (scv_scratch->get(stream, offW + (size_t)nPix * 2 * Q * sizeof(float), (void**)&base)) return 1;
  a.partA = (double*)base;
  a.partB = (double*)(base + offB);
  a.W = (float*)(base + offW);
  switch (Q) {
    case 1: launch_scv<1>(a, pixels, reduce, st); break;
    case 2: launch_scv<2>(a, pixels, reduce, st); break;
    case 3: launch_scv<3>(a, pixels, reduce, st); break;
    case 4: launch_scv<4>(a, pixels, reduce, st); break;
    case 5: launch_scv<5>(a, pixels, reduce, st); break;
    case 6: launch_scv<6>(a, pixels, reduce, st); break;
    case 7: launch_scv<7>(a, pixels, reduce, st); break;
    default: launch_scv<8>(a, pixels, reduce, st); break;
  }
  RTX_LAUNCH_CHECK();
  if (pixels) {
    const long long n = nPix * (nMix + 1);
    hipLaunchKernelGGL(scv_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    RTX_LAUNCH_CHECK();
  }
  if (reduce) {
    const long long n = (long long)(nEnd + 1) * Q * nB;
    hipLaunchKernelGGL(scv_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, Q);
    RTX_LAUNCH_CHECK();
  }
  return 0;
}
