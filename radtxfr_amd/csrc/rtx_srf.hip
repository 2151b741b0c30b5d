// Band averages under tabulated spectral response functions (include/radtxfr_hip.h, rtx_srf_apply):
//
//   Y_out[b][s] = sum_i R_b(X_i) D_i Y[i][s]  /  sum_i R_b(X_i) D_i
//
// R_b: the piecewise-linear function through band b's knots, 0 outside [x_first, x_last], both ends included;
// D_i: the trapezoid cell of axis point i. The definition is this project's own (the reference has only the MAKO shapes).
//
// Structure, after ils_rows_kernel (rtx_radiance.hip): a workgroup owns SRF_CH consecutive rows of Y x 1024 columns, reads
// them once and keeps the sums of the bands that reach its chunk; a second kernel adds a band's chunk sums in ascending
// chunk order and normalises. The bands of a call are taken SRF_SLOTS at a time (three launches per group), so a band's
// slot in the workspace is its index in the group: no list of bands per chunk, no overflow, no atomics. A workgroup whose
// chunk no band of the group reaches returns before it reads anything, so Y is read once where the bands of a group lie
// side by side (band lists sorted by wavenumber: the usual case) and never more often than bands cover a row.
//
// Determinism: Y_out[b][s] is a pure function of (axis, band b's knots, column s of Y). The weight of row i under band b
// is computed in fp64 from the axis and the band's own knots and rounded to fp32 once; a (band, chunk, column) sum is ONE
// fp32 fmaf chain over the chunk's rows in ascending order, whatever lane, wave or load width carries it and whichever
// other bands share the pass (a row of weight 0 is skipped, not multiplied); the chunk sums are added in fp64 in
// ascending chunk order. Chunks are cut at multiples of SRF_CH from the axis' first point.
#include "rtx_srf_common.h"

#define SRF_CAP 4           // bands per pass over the chunk's rows: their weights are one float4 per row in LDS

__global__ __launch_bounds__(64) void srf_support_kernel(SrfArgs a) {
  const int j = threadIdx.x;
  if (j >= a.ng) return;
  const double x_first = a.kx[a.ks[j]], x_last = a.kx[a.ks[j + 1] - 1];
  a.sup[2 * j] = srf_bound(a, x_first, 0);
  a.sup[2 * j + 1] = srf_bound(a, x_last, 1);
}

// VEC: 16-byte loads of Y (nS % 4 == 0, ldY % 4 == 0, 16-byte aligned); else point by point. The arithmetic is the same.
template <bool VEC>
__device__ __forceinline__ float4 srf_load(const SrfArgs& a, long long row, long long col4) {
  if (VEC) return reinterpret_cast<const float4*>(a.Y + row * a.ldY)[col4];
  const float* y = a.Y + row * a.ldY;
  const long long c = 4 * col4;
  float4 v;
  v.x = y[c];  // col4 is live: c < nS
  v.y = c + 1 < a.nS ? y[c + 1] : 0.f;
  v.z = c + 2 < a.nS ? y[c + 2] : 0.f;
  v.w = c + 3 < a.nS ? y[c + 3] : 0.f;
  return v;
}

template <bool VEC>
__device__ __forceinline__ void srf_store(const SrfArgs& a, float* p, long long col4, float4 v) {
  if (VEC) { reinterpret_cast<float4*>(p)[col4] = v; return; }
  const long long c = 4 * col4;
  p[c] = v.x;
  if (c + 1 < a.nS) p[c + 1] = v.y;
  if (c + 2 < a.nS) p[c + 2] = v.z;
  if (c + 3 < a.nS) p[c + 3] = v.w;
}

// a row of weight 0 leaves the sum alone (not fmaf(0, y, acc): a non-finite y under another band must not reach this one)
__device__ __forceinline__ void srf_fma(float4& acc, float w, const float4& y) {
  const bool on = w != 0.f;
  acc.x = on ? fmaf(w, y.x, acc.x) : acc.x;
  acc.y = on ? fmaf(w, y.y, acc.y) : acc.y;
  acc.z = on ? fmaf(w, y.z, acc.z) : acc.z;
  acc.w = on ? fmaf(w, y.w, acc.w) : acc.w;
}

template <bool VEC>
__global__ __launch_bounds__(256) void srf_rows_kernel(SrfArgs a) {
  const long long chunk = blockIdx.x;
  const long long r0 = chunk * SRF_CH, r1 = r0 + SRF_CH < a.nx ? r0 + SRF_CH : a.nx;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long col4 = (long long)blockIdx.y * 256 + threadIdx.x, n4 = (a.nS + 3) >> 2;
  const bool live = col4 < n4;
  __shared__ float4 s_w[SRF_CH + 4];        // the pass's SRF_CAP weights of every row of the chunk (+ zeros behind)
  __shared__ double s_kx[SRF_MAX_KNOTS];    // one band's knots under the chunk
  __shared__ float s_kr[SRF_MAX_KNOTS];
  __shared__ int s_lo[SRF_SLOTS], s_hi[SRF_SLOTS];  // support of band j within the chunk as rows [lo, hi) from r0; empty: lo >= hi
  __shared__ int s_any;
  if (threadIdx.x == 0) s_any = 0;
  __syncthreads();
  if (threadIdx.x < SRF_SLOTS) {
    int lo = 0, hi = 0;
    if (threadIdx.x < a.ng) {
      const long long L = a.sup[2 * threadIdx.x], H = a.sup[2 * threadIdx.x + 1];
      const long long l = L > r0 ? L : r0, h = H < r1 ? H : r1;
      if (h > l) { lo = (int)(l - r0); hi = (int)(h - r0); s_any = 1; }
    }
    s_lo[threadIdx.x] = lo; s_hi[threadIdx.x] = hi;
  }
  __syncthreads();
  if (!s_any) return;  // no band of the group reaches this chunk: nothing is read
  float* wcomp = reinterpret_cast<float*>(s_w);
  for (int j0 = 0; j0 < a.ng; j0 += SRF_CAP) {
    int ra = SRF_CH, rb = 0;  // rows of the chunk under any band of the pass
#pragma unroll
    for (int u = 0; u < SRF_CAP; ++u)
      if (s_hi[j0 + u] > s_lo[j0 + u]) { ra = min(ra, s_lo[j0 + u]); rb = max(rb, s_hi[j0 + u]); }
    if (rb <= ra) continue;  // uniform over the workgroup
    // ---- weights: thread t takes rows t, t + 256, ... of the chunk and walks along the band's segments with them
    for (int u = 0; u < SRF_CAP; ++u) {
      const int j = j0 + u;
      const bool act = s_hi[j] > s_lo[j];  // uniform; j < SRF_SLOTS, and a slot past the group is empty
      int jA = 0, m = 0, lo = 0, hi = 0;
      if (act) {
        lo = s_lo[j]; hi = s_hi[j];
        const double* kx = a.kx + a.ks[j];
        const int nk = a.ks[j + 1] - a.ks[j];
        jA = srf_segment(kx, nk, srf_x(a, r0 + lo));
        m = srf_segment(kx, nk, srf_x(a, r0 + hi - 1)) + 2 - jA;  // knots jA .. jB + 1
        for (int q = threadIdx.x; q < m; q += 256) { s_kx[q] = kx[jA + q]; s_kr[q] = a.kr[a.ks[j] + jA + q]; }
      }
      __syncthreads();
      int seg = 0;
      for (int t = threadIdx.x; t < SRF_CH + 4; t += 256) {
        float w = 0.f;
        if (act && t >= lo && t < hi) {
          const double x = srf_x(a, r0 + t);
          while (seg + 2 < m && x >= s_kx[seg + 1]) ++seg;
          const double xa = s_kx[seg], xb = s_kx[seg + 1], ya = (double)s_kr[seg], yb = (double)s_kr[seg + 1];
          const double R = (yb - ya) / (xb - xa) * (x - xa) + ya;
          w = (float)(fmax(R, 0.0) * srf_delta(a, r0 + t));
        }
        wcomp[4 * t + u] = w;
      }
      __syncthreads();  // the weights are written and the knots read before the next band is staged
    }
    // ---- the chunk's sums of the weights: wave u adds band u's, lanes over rows, in a fixed order
    {
      double v = 0.0;
      for (int t = lane; t < SRF_CH; t += 64) v += (double)wcomp[4 * t + wave];
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
      const int j = j0 + wave;
      if (blockIdx.y == 0 && lane == 0 && s_hi[j] > s_lo[j]) a.W[chunk * SRF_SLOTS + j] = v;
    }
    // ---- rows: every thread owns four columns and runs each band's sum as one chain over the rows, ascending
    if (live) {
      float4 acc[SRF_CAP];
#pragma unroll
      for (int u = 0; u < SRF_CAP; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int t = ra; t < rb; t += 4) {  // four rows in flight
        float4 y[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) y[q] = t + q < rb ? srf_load<VEC>(a, r0 + t + q, col4) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 w = s_w[t + q];  // one address for the whole wave; zeros from rb on
          srf_fma(acc[0], w.x, y[q]); srf_fma(acc[1], w.y, y[q]); srf_fma(acc[2], w.z, y[q]); srf_fma(acc[3], w.w, y[q]);
        }
      }
#pragma unroll
      for (int u = 0; u < SRF_CAP; ++u) {
        const int j = j0 + u;
        if (s_hi[j] > s_lo[j])
          srf_store<VEC>(a, a.P + (size_t)(chunk * SRF_SLOTS + j) * (size_t)a.nS, col4, acc[u]);
      }
    }
    __syncthreads();  // s_w is rewritten by the next pass
  }
}

// one thread per (band, column): the band's chunk sums in ascending chunk order, in fp64, then the quotient
__global__ __launch_bounds__(256) void srf_reduce_kernel(SrfArgs a) {
  const int j = blockIdx.x;
  const long long col = (long long)blockIdx.y * 256 + threadIdx.x;
  if (col >= a.nS) return;
  const long long lo = a.sup[2 * j], hi = a.sup[2 * j + 1];
  double acc = 0.0, N = 0.0;
  if (hi > lo) {
    for (long long ch = lo / SRF_CH; ch <= (hi - 1) / SRF_CH; ++ch) {
      acc += (double)a.P[(size_t)(ch * SRF_SLOTS + j) * (size_t)a.nS + col];
      N += a.W[ch * SRF_SLOTS + j];
    }
  }
  a.Yout[(size_t)j * a.nS + col] = (float)(acc / N);  // a denominator of 0: 0/0 = NaN, like rtx_ils' empty band
  if (a.wsum && col == 0) a.wsum[j] = (float)N;
}

// workspace per (device, stream), like rtx_ils': calls on one stream are ordered by it, calls on different streams must
// not share chunk sums.
static StreamScratch* const srf_scratch = new StreamScratch();

extern "C" int rtx_srf_chunk_points(void) { return SRF_CH; }
extern "C" int rtx_srf_max_knots(void) { return SRF_MAX_KNOTS; }

extern "C" int rtx_srf_apply(const rtx_grid* grid, const double* X, int64_t nx, const float* Y, int64_t nS, int64_t ldY, int nB,
                             const int32_t* knot_start_h, const double* knot_x_d, const float* knot_r_d, float* Y_out,
                             float* wsum_out, void* stream) {
  if (!X) {
    if (!grid) RTX_FAIL("neither an axis nor a grid");
    if (rtx_check_grid(grid)) return 1;
    if (nx != grid->n) RTX_FAIL("nx=%lld != grid->n=%lld", (long long)nx, (long long)grid->n);
  }
  if (nB < 0 || nS < 0 || nx < 0) RTX_FAIL("negative size");
  if (nB == 0 || nS == 0) return 0;
  if (!Y || !knot_start_h || !knot_x_d || !knot_r_d || !Y_out) RTX_FAIL("a required pointer is NULL");
  if (ldY < nS) RTX_FAIL("ldY=%lld < nS=%lld", (long long)ldY, (long long)nS);
  if (knot_start_h[0] < 0) RTX_FAIL("knot_start[0]=%d is negative", (int)knot_start_h[0]);
  for (int b = 0; b < nB; ++b) {
    const long long nk = (long long)knot_start_h[b + 1] - (long long)knot_start_h[b];
    if (nk < 0) RTX_FAIL("knot_start is not ascending at band %d", b);
    if (nk < 2) RTX_FAIL("band %d has %lld knots: a response table needs at least 2", b, nk);
    if (nk > SRF_MAX_KNOTS) RTX_FAIL("band %d has %lld knots: at most %d", b, nk, SRF_MAX_KNOTS);
  }
  const long long n_chunks = (nx + SRF_CH - 1) / SRF_CH;
  if (n_chunks > 0x7fffffffLL) RTX_FAIL("nx=%lld: too many chunks", (long long)nx);
  const long long ncb = ((nS + 3) / 4 + 255) / 256;  // column blocks of the row kernel
  if (ncb > 65535) RTX_FAIL("nS=%lld: too many columns for one call", (long long)nS);
  hipStream_t st = (hipStream_t)stream;
  const size_t nW = (size_t)n_chunks * SRF_SLOTS, nP = nW * (size_t)nS;
  void* base = nullptr;
  if (srf_scratch->get(st, nW * sizeof(double) + 2 * SRF_SLOTS * sizeof(long long) + nP * sizeof(float), &base)) return 1;
  SrfArgs a;
  if (grid) a.g = to_dev(grid); else { a.g.xmin = a.g.xmax = a.g.step = 0; a.g.n_total = a.g.offset = a.g.n = 0; }
  a.X = X; a.nx = nx; a.nS = nS; a.ldY = ldY; a.Y = Y; a.kx = knot_x_d; a.kr = knot_r_d;
  a.W = (double*)base; a.sup = (long long*)(a.W + nW); a.P = (float*)(a.sup + 2 * SRF_SLOTS);
  const bool vec = nS % 4 == 0 && ldY % 4 == 0 && (uintptr_t)Y % 16 == 0;
  for (int g0 = 0; g0 < nB; g0 += SRF_SLOTS) {
    a.ng = nB - g0 < SRF_SLOTS ? nB - g0 : SRF_SLOTS;
    for (int j = 0; j <= SRF_SLOTS; ++j) a.ks[j] = knot_start_h[g0 + (j < a.ng ? j : a.ng)];
    a.Yout = Y_out + (size_t)g0 * (size_t)nS;
    a.wsum = wsum_out ? wsum_out + g0 : nullptr;
    hipLaunchKernelGGL(srf_support_kernel, dim3(1), dim3(64), 0, st, a);
    RTX_LAUNCH_CHECK();
    if (n_chunks > 0) {
      if (vec) hipLaunchKernelGGL(srf_rows_kernel<true>, dim3((unsigned)n_chunks, (unsigned)ncb), dim3(256), 0, st, a);
      else hipLaunchKernelGGL(srf_rows_kernel<false>, dim3((unsigned)n_chunks, (unsigned)ncb), dim3(256), 0, st, a);
      RTX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(srf_reduce_kernel, dim3((unsigned)a.ng, (unsigned)((nS + 255) / 256)), dim3(256), 0, st, a);
    RTX_LAUNCH_CHECK();
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------
// Fused band radiances under response tables (include/radtxfr_hip.h, rtx_srf_moments): the moments
//   N_b = sum_i w,  C_b = sum_i w (tau Ld + La),  M[t][b][j] = sum_i w tau (B(nu_i, Ts_t) - Ld) hat_j(nu_i),  w = R_b(X_i) D_i
// that rtx_band_mix turns into (C_b + sum_j M[t][b][j] E[j][k]) / N_b. Nothing of size nX * nE is formed.
//
// Structure, after srf_rows_kernel: a workgroup owns the SRF_CH points of a chunk and the bands of a launch group that reach
// it. It reads tau / La / Ld once, evaluates Planck once per (point, temperature) and parks tau (B - Ld), tau Ld + La and
// every point's knot interval and interpolation weight in LDS; then, band by band, it stages the band's weights as
// srf_rows_kernel does and hands out one task per (sub-chunk of SRFM_SUB points, knot the sub-chunk touches, temperature):
// a thread adds the task's points in ascending order in one fp32 fmaf chain of at most SRFM_SUB terms. Knots a few
// points apart (finer than the grid) make many short tasks, knots a thousand points apart few long ones: one path for both.
// A second kernel adds a knot's sub-chunk sums in ascending order in fp64.
//
// Workspace row of a (band slot, temperature): the sum of sub-chunk s (counted from the grid's first point) for knot j is
// element j + 2 s. Sub-chunk s touches the knots [ja(s), jb(s)] = [interval of its first point, interval of its last point
// + 1], and jb(s) <= ja(s + 1) + 1, so no two sub-chunks share an element: no offsets table, no atomics.
#define SRFM_SUB 64                     // points per sub-chunk = the longest fp32 chain
#define SRFM_NSUB (SRF_CH / SRFM_SUB)   // sub-chunks per chunk
#define SRFM_MAXT 8                     // temperatures per call: their tau (B - Ld) are SRFM_MAXT x 4 KiB of LDS

struct SrfmArgs {
  SrfArgs s;  // g, nx, kx, kr, ng, ks, sup as in rtx_srf_apply; X = NULL (uniform grid), the rest unused
  const float *tau, *La, *Ld;
  const double* Xk;
  long long nk;
  int nT, nB;                          // nB: bands of the whole call (M_out's stride)
  double c2l2e_over_T[SRFM_MAXT];      // 100 c2 log2(e) / Ts_t
  long long row;                       // elements per workspace row: nk + 2 * (sub-chunks of the grid)
  double *WN, *WC;                     // [n_chunks][SRF_SLOTS] chunk sums of w and of w (tau Ld + La)
  float* P;                            // [SRF_SLOTS][nT][row] sub-chunk sums
  float *N, *C, *M;                    // the group's first band in N_out, C_out, M_out[0]
  int2* jrange;
};

// supports as srf_support_kernel, and the first and last knot each band touches: a point with c knots <= x lies in
// interval c - 1 and touches knots max(c - 1, 0) and min(c, nk - 1) (np.interp holds the end values outside the knots)
__global__ __launch_bounds__(64) void srfm_support_kernel(SrfmArgs a) {
  const int j = threadIdx.x;
  if (j >= a.s.ng) return;
  const double x_first = a.s.kx[a.s.ks[j]], x_last = a.s.kx[a.s.ks[j + 1] - 1];
  const long long lo = srf_bound(a.s, x_first, 0), hi = srf_bound(a.s, x_last, 1);
  a.s.sup[2 * j] = lo;
  a.s.sup[2 * j + 1] = hi;
  int2 jr = make_int2(0, -1);  // no point under the band: an empty range
  if (hi > lo) {
    const long long c0 = srfm_count(a.Xk, a.nk, srf_x(a.s, lo)), c1 = srfm_count(a.Xk, a.nk, srf_x(a.s, hi - 1));
    jr.x = (int)(c0 > 0 ? c0 - 1 : 0);
    jr.y = (int)(c1 < a.nk - 1 ? c1 : a.nk - 1);
  }
  a.jrange[j] = jr;
}

__global__ __launch_bounds__(256) void srfm_chunk_kernel(SrfmArgs a) {
  const long long chunk = blockIdx.x;
  const long long r0 = chunk * SRF_CH, r1 = r0 + SRF_CH < a.s.nx ? r0 + SRF_CH : a.s.nx;
  const int np = (int)(r1 - r0);  // points of this chunk
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ float s_g[SRFM_MAXT][SRF_CH];  // tau (B(Ts_t) - Ld)
  __shared__ float s_c[SRF_CH];             // tau Ld + La
  __shared__ float2 s_h[SRF_CH];            // the point's weights on knots j0 and j0 + 1 (srfm_hats; (1, 0) outside the knots)
  __shared__ int s_j0[SRF_CH];              // its lower knot; past the grid's end: INT_MAX
  __shared__ float s_w[SRF_CH];             // one band's weights
  __shared__ double s_kx[SRF_MAX_KNOTS];    // one band's knots under the chunk
  __shared__ float s_kr[SRF_MAX_KNOTS];
  __shared__ int s_lo[SRF_SLOTS], s_hi[SRF_SLOTS];  // support of band j within the chunk as rows [lo, hi) from r0
  __shared__ int s_ja[SRFM_NSUB], s_kn[SRFM_NSUB], s_koff[SRFM_NSUB + 1];  // first knot, knots and task offset of a sub-chunk
  __shared__ double s_red[2][4];
  __shared__ int s_any;
  if (threadIdx.x == 0) s_any = 0;
  __syncthreads();
  if (threadIdx.x < SRF_SLOTS) {
    int lo = 0, hi = 0;
    if (threadIdx.x < a.s.ng) {
      const long long L = a.s.sup[2 * threadIdx.x], H = a.s.sup[2 * threadIdx.x + 1];
      const long long l = L > r0 ? L : r0, h = H < r1 ? H : r1;
      if (h > l) { lo = (int)(l - r0); hi = (int)(h - r0); s_any = 1; }
    }
    s_lo[threadIdx.x] = lo; s_hi[threadIdx.x] = hi;
  }
  __syncthreads();
  if (!s_any) return;  // no band of the group reaches this chunk: nothing is read
  int ua = SRF_CH, ub = 0;  // rows under any band of the group: Planck is evaluated there only
  for (int j = 0; j < SRF_SLOTS; ++j)
    if (s_hi[j] > s_lo[j]) { ua = min(ua, s_lo[j]); ub = max(ub, s_hi[j]); }
  // ---- the chunk's points: thread t takes rows 4 t .. 4 t + 3 (one 16-byte load per array where it can)
  {
    const int p0 = 4 * threadIdx.x;
    float tt[4] = {0.f, 0.f, 0.f, 0.f}, la[4] = {0.f, 0.f, 0.f, 0.f}, ld[4] = {0.f, 0.f, 0.f, 0.f};
    const bool vec = (((uintptr_t)a.tau | (uintptr_t)a.La | (uintptr_t)a.Ld) & 15) == 0;  // r0 is a multiple of 4
    if (vec && p0 + 3 < np) {
      const float4 t4 = *reinterpret_cast<const float4*>(a.tau + r0 + p0), a4 = *reinterpret_cast<const float4*>(a.La + r0 + p0),
                   d4 = *reinterpret_cast<const float4*>(a.Ld + r0 + p0);
      tt[0] = t4.x; tt[1] = t4.y; tt[2] = t4.z; tt[3] = t4.w;
      la[0] = a4.x; la[1] = a4.y; la[2] = a4.z; la[3] = a4.w;
      ld[0] = d4.x; ld[1] = d4.y; ld[2] = d4.z; ld[3] = d4.w;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (p0 + q < np) { tt[q] = a.tau[r0 + p0 + q]; la[q] = a.La[r0 + p0 + q]; ld[q] = a.Ld[r0 + p0 + q]; }
    }
    long long cnt = p0 < np ? srfm_count(a.Xk, a.nk, srf_x(a.s, r0 + p0)) : 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int p = p0 + q;
      int j0 = 0x7fffffff;
      float h0 = 1.f, h1 = 0.f, c = 0.f;
      if (p < np) {
        const double x = srf_x(a.s, r0 + p);
        while (cnt < a.nk && a.Xk[cnt] <= x) ++cnt;  // the knots ascend with the rows
        j0 = (int)(cnt > 0 ? cnt - 1 : 0);
        if (cnt > 0 && cnt < a.nk) srfm_hats(x, a.Xk[cnt - 1], a.Xk[cnt], h0, h1);
        c = fmaf(tt[q], ld[q], la[q]);
        const bool under = p >= ua && p < ub;
        const double x100 = x * 100.0;
        const double c1x3 = RT_C1 * (x100 * x100 * x100) * 1e4;
        for (int t = 0; t < a.nT; ++t)
          s_g[t][p] = under ? tt[q] * (planck_f32(c1x3, x, a.c2l2e_over_T[t]) - ld[q]) : 0.f;
      } else {
        for (int t = 0; t < a.nT; ++t) s_g[t][p] = 0.f;
      }
      s_j0[p] = j0; s_h[p] = make_float2(h0, h1); s_c[p] = c;
    }
  }
  __syncthreads();
  if (threadIdx.x < SRFM_NSUB) {  // the knots a sub-chunk touches: lower knot of its first point .. upper knot of its last
    const int first = SRFM_SUB * threadIdx.x, last = min(first + SRFM_SUB, np) - 1;
    int ja = 0, kn = 0;
    if (first < np) {
      ja = s_j0[first];
      const long long jb = min((long long)s_j0[last] + 1, a.nk - 1);
      kn = (int)(jb - ja + 1);
    }
    s_ja[threadIdx.x] = ja; s_kn[threadIdx.x] = kn;
  }
  __syncthreads();
  if (threadIdx.x <= SRFM_NSUB) {
    int off = 0;
    for (int s = 0; s < (int)threadIdx.x; ++s) off += s_kn[s];
    s_koff[threadIdx.x] = off;
  }
  __syncthreads();
  const int ntask = s_koff[SRFM_NSUB] * a.nT;
  for (int j = 0; j < a.s.ng; ++j) {
    const int lo = s_lo[j], hi = s_hi[j];
    if (hi <= lo) continue;  // uniform over the workgroup
    // ---- the band's weights, as srf_rows_kernel forms them
    {
      const double* kx = a.s.kx + a.s.ks[j];
      const int nkb = a.s.ks[j + 1] - a.s.ks[j];
      const int jA = srf_segment(kx, nkb, srf_x(a.s, r0 + lo));
      const int m = srf_segment(kx, nkb, srf_x(a.s, r0 + hi - 1)) + 2 - jA;  // knots jA .. jB + 1
      for (int q = threadIdx.x; q < m; q += 256) { s_kx[q] = kx[jA + q]; s_kr[q] = a.s.kr[a.s.ks[j] + jA + q]; }
      __syncthreads();
      int seg = 0;
      for (int t = threadIdx.x; t < SRF_CH; t += 256)
        s_w[t] = t >= lo && t < hi ? srf_weight(a.s, s_kx, s_kr, m, seg, r0 + t) : 0.f;
      __syncthreads();
    }
    // ---- the chunk's N and C in fp64: a thread's four rows, the lanes of a wave, the four waves, always in this order
    {
      double n = 0.0, c = 0.0;
      for (int t = threadIdx.x; t < SRF_CH; t += 256) {
        const double w = (double)s_w[t];
        if (w != 0.0) { n += w; c += w * (double)s_c[t]; }  // a row of weight 0 is skipped, not multiplied
      }
      for (int off = 32; off > 0; off >>= 1) { n += __shfl_down(n, off); c += __shfl_down(c, off); }
      if (lane == 0) { s_red[0][wave] = n; s_red[1][wave] = c; }
      __syncthreads();
      if (threadIdx.x == 0) {
        a.WN[chunk * SRF_SLOTS + j] = (s_red[0][0] + s_red[0][1]) + (s_red[0][2] + s_red[0][3]);
        a.WC[chunk * SRF_SLOTS + j] = (s_red[1][0] + s_red[1][1]) + (s_red[1][2] + s_red[1][3]);
      }
    }
    // ---- knot sums: task = (sub-chunk, knot it touches, temperature), temperature fastest
    for (int task = threadIdx.x; task < ntask; task += 256) {
      const int t = task % a.nT, kk = task / a.nT;
      int s = 0;
      while (kk >= s_koff[s + 1]) ++s;
      const int b0 = max(SRFM_SUB * s, lo), b1 = min(SRFM_SUB * (s + 1), hi);
      if (b1 <= b0) continue;  // the band does not reach this sub-chunk: its elements are neither written nor read
      const int jk = s_ja[s] + (kk - s_koff[s]);
      int u = b0, v = b1;  // [u, e): the rows of [b0, b1) whose lower knot is jk - 1 or jk (the lower knots ascend)
      while (u < v) {
        const int mid = (u + v) >> 1;
        if (s_j0[mid] >= jk - 1) v = mid; else u = mid + 1;
      }
      int e = u;
      v = b1;
      while (e < v) {
        const int mid = (e + v) >> 1;
        if (s_j0[mid] > jk) v = mid; else e = mid + 1;
      }
      float acc = 0.f;
#pragma unroll 4
      for (int i = u; i < e; ++i) {  // a counted loop: the LDS reads of the rows ahead do not wait for the chain
        const float w = s_w[i];
        const float2 h = s_h[i];
        const float hat = s_j0[i] == jk ? h.x : h.y;
        const float term = fmaf(w * s_g[t][i], hat, acc);
        acc = w != 0.f ? term : acc;  // a row of weight 0 is skipped, not multiplied
      }
      a.P[((size_t)j * a.nT + t) * (size_t)a.row + (size_t)jk + 2 * (size_t)(chunk * SRFM_NSUB + s)] = acc;
    }
    __syncthreads();  // s_w, the knots and s_red are rewritten by the next band
  }
}

// one thread per (temperature, knot) of a band: the knot's sub-chunk sums in ascending order, in fp64. The sub-chunks that
// hold a sum for knot j are those with a point in [Xk[j - 1], Xk[j + 1]) (the ends: everything below / above) under the band.
__global__ __launch_bounds__(256) void srfm_reduce_kernel(SrfmArgs a) {
  const int j = blockIdx.x;
  const long long q = (long long)blockIdx.y * 256 + threadIdx.x;
  if (q >= a.nk * a.nT) return;
  const int t = (int)(q / a.nk);
  const long long jk = q - (long long)t * a.nk;
  const long long lo = a.s.sup[2 * j], hi = a.s.sup[2 * j + 1];
  const int2 jr = a.jrange[j];
  double acc = 0.0;
  if (hi > lo && jk >= jr.x && jk <= jr.y) {
    long long sA = lo / SRFM_SUB, sB = (hi - 1) / SRFM_SUB;
    if (jk >= 2) sA = max(sA, srf_bound(a.s, a.Xk[jk - 1], 0) / SRFM_SUB);
    if (jk <= a.nk - 2) {
      const long long p = srf_bound(a.s, a.Xk[jk + 1], 0);  // rows from p on lie in interval jk + 1 or above
      sB = p > 0 ? min(sB, (p - 1) / SRFM_SUB) : -1;
    }
    const float* row = a.P + ((size_t)j * a.nT + t) * (size_t)a.row + (size_t)jk;
    for (long long s = sA; s <= sB; ++s) acc += (double)row[2 * s];
  }
  a.M[((size_t)t * a.nB + j) * (size_t)a.nk + jk] = (float)acc;  // 0 on the knots the band does not touch
  if (q == 0) {
    double N = 0.0, C = 0.0;
    if (hi > lo) {
      for (long long ch = lo / SRF_CH; ch <= (hi - 1) / SRF_CH; ++ch) {
        N += a.WN[ch * SRF_SLOTS + j];
        C += a.WC[ch * SRF_SLOTS + j];
      }
    }
    a.N[j] = (float)N;  // 0 with C = 0 where no point lies under the band: rtx_band_mix divides 0 by 0, NaN
    a.C[j] = (float)C;
  }
}

extern "C" int rtx_srf_moments_max_temps(void) { return SRFM_MAXT; }

extern "C" int rtx_srf_moments(const rtx_grid* grid, const float* tau, const float* La, const float* Ld, const double* Ts_h, int nT,
                               const double* Xk, int64_t nk, int nB, const int32_t* knot_start_h, const double* knot_x_d,
                               const float* knot_r_d, float* N_out, float* C_out, float* M_out, int32_t* jrange_out, void* stream) {
  if (!grid) RTX_FAIL("no grid");
  if (rtx_check_grid(grid)) return 1;
  if (nk < 1) RTX_FAIL("nk=%lld: need at least 1 emissivity knot", (long long)nk);
  if (nk > (1ll << 23)) RTX_FAIL("nk=%lld: at most %lld emissivity knots", (long long)nk, 1ll << 23);
  if (nT < 1 || nT > SRFM_MAXT) RTX_FAIL("nT=%d outside [1,%d]", nT, SRFM_MAXT);
  if (nB < 0) RTX_FAIL("negative size");
  if (nB == 0) return 0;
  if (!tau || !La || !Ld || !Ts_h || !Xk || !knot_start_h || !knot_x_d || !knot_r_d || !N_out || !C_out || !M_out || !jrange_out)
    RTX_FAIL("a required pointer is NULL");
  for (int t = 0; t < nT; ++t)
    if (!(Ts_h[t] > 0.0)) RTX_FAIL("surface temperature %g", Ts_h[t]);
  if (knot_start_h[0] < 0) RTX_FAIL("knot_start[0]=%d is negative", (int)knot_start_h[0]);
  for (int b = 0; b < nB; ++b) {
    const long long n = (long long)knot_start_h[b + 1] - (long long)knot_start_h[b];
    if (n < 0) RTX_FAIL("knot_start is not ascending at band %d", b);
    if (n < 2) RTX_FAIL("band %d has %lld knots: a response table needs at least 2", b, n);
    if (n > SRF_MAX_KNOTS) RTX_FAIL("band %d has %lld knots: at most %d", b, n, SRF_MAX_KNOTS);
  }
  const long long nx = grid->n;
  const long long n_chunks = (nx + SRF_CH - 1) / SRF_CH;
  if (n_chunks > 0x7fffffffLL / SRFM_NSUB) RTX_FAIL("grid->n=%lld: too many chunks", nx);
  const long long nqb = ((long long)nk * nT + 255) / 256;  // blocks of the reduce kernel per band
  if (nqb > 65535) RTX_FAIL("nk=%lld x nT=%d: too many for one call", (long long)nk, nT);
  hipStream_t st = (hipStream_t)stream;
  SrfmArgs a;
  a.row = (long long)nk + 2 * n_chunks * SRFM_NSUB;
  const size_t nW = (size_t)n_chunks * SRF_SLOTS, nP = (size_t)SRF_SLOTS * (size_t)nT * (size_t)a.row;
  void* base = nullptr;
  if (srf_scratch->get(st, 2 * nW * sizeof(double) + 2 * SRF_SLOTS * sizeof(long long) + nP * sizeof(float), &base)) return 1;
  a.s.g = to_dev(grid);
  a.s.X = nullptr; a.s.nx = nx; a.s.nS = 0; a.s.ldY = 0; a.s.Y = nullptr; a.s.kx = knot_x_d; a.s.kr = knot_r_d;
  a.s.P = nullptr; a.s.W = nullptr; a.s.Yout = nullptr; a.s.wsum = nullptr;
  a.WN = (double*)base; a.WC = a.WN + nW; a.s.sup = (long long*)(a.WC + nW); a.P = (float*)(a.s.sup + 2 * SRF_SLOTS);
  a.tau = tau; a.La = La; a.Ld = Ld; a.Xk = Xk; a.nk = nk; a.nT = nT; a.nB = nB;
  for (int t = 0; t < SRFM_MAXT; ++t) a.c2l2e_over_T[t] = t < nT ? 100.0 * RT_C2 * LOG2E / Ts_h[t] : 0.0;
  for (int g0 = 0; g0 < nB; g0 += SRF_SLOTS) {
    a.s.ng = nB - g0 < SRF_SLOTS ? nB - g0 : SRF_SLOTS;
    for (int j = 0; j <= SRF_SLOTS; ++j) a.s.ks[j] = knot_start_h[g0 + (j < a.s.ng ? j : a.s.ng)];
    a.N = N_out + g0; a.C = C_out + g0; a.M = M_out + (size_t)g0 * (size_t)nk;
    a.jrange = reinterpret_cast<int2*>(jrange_out) + g0;
    hipLaunchKernelGGL(srfm_support_kernel, dim3(1), dim3(64), 0, st, a);
    RTX_LAUNCH_CHECK();
    if (n_chunks > 0) {
      hipLaunchKernelGGL(srfm_chunk_kernel, dim3((unsigned)n_chunks), dim3(256), 0, st, a);
      RTX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(srfm_reduce_kernel, dim3((unsigned)a.s.ng, (unsigned)nqb), dim3(256), 0, st, a);
    RTX_LAUNCH_CHECK();
  }
  return 0;
}
