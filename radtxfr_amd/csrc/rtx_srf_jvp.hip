// Tangent of the fused band radiances under response tables (include/radtxfr_hip.h, rtx_srf_radiance_jvp):
// rtx_srf_moments + rtx_band_mix carried along tangent vectors. With w = R_b(X_i) D_i, N_b = sum_i w, hat_j np.interp's hats
// on Xk and, per vector, tangents d_tau, d_La, d_Ld on the native grid, dTs[t] and dE[j][e],
//   c'_i   = d_tau_i Ld_i + tau_i d_Ld_i + d_La_i
//   m'_t,i = d_tau_i (B(nu_i, Ts_t) - Ld_i) + tau_i (dB/dT(nu_i, Ts_t) dTs_t - d_Ld_i)
//   C'_b = sum_i w c'_i,   M'[t][b][j] = sum_i w m'_t,i hat_j(nu_i)
//   dL[t][b][e] = (C'_b + sum_j M'[t][b][j] E[j][e] + sum_j M[t][b][j] dE[j][e]) / N_b,   j over jrange[b],
// M, N and jrange the forward's own outputs. Nothing of size nX * nE is formed: a second set of moments, then a contraction.
//
// Structure, after srfm_chunk_kernel (rtx_srf.hip):
//   srfj_support_kernel  per band of a launch group: its support [lo, hi) on the grid
//   srfj_chunk_kernel    one workgroup per chunk of SRF_CH points, ONE LANE PER POINT. A chunk no band of the group reaches
//                        returns before it reads anything. A lane reads tau and Ld once, searches its knot interval once,
//                        evaluates B and dB/dT once per temperature and parks c' (per vector) and m' (per vector and
//                        temperature) in LDS as fp64: the vectors of a launch share all of that. Then, band by band, the
//                        weights (srf_weight: the forward's fp32 number), the chunk's sum of w c', and one task per
//                        (sub-chunk of SRFJ_SUB points, knot it touches, vector, temperature) that adds its points in
//                        ascending order.
//   srfj_reduce_kernel   per (band, vector, temperature, knot): the sub-chunk sums in ascending order; per (band, vector)
//                        the chunk sums of w c' in ascending order
//   srfj_mix_kernel      per (band, column, vector, temperature): dL, over jrange[b] only
// Workspace row of a (band slot, vector, temperature): rtx_srf_moments' (element j + 2 s for knot j and sub-chunk s), in fp64.
//
// Arithmetic: c' and m' are formed in fp64 from the fp32 inputs, fp32 B and fp32 dB/dT (planck_dT), left to right as
// written above, no fused operation. w is the forward's fp32 weight and the hats its fp32 pair (srfm_hats); every product with
// them is fp64, (w m') hat, and so is every sum: the points of a sub-chunk ascending (a row of weight 0 is skipped, not
// multiplied), the sub-chunks ascending; w c' over the 64 lanes of a wave by a shuffle-down tree, the 16 waves in wave
// order, the chunks ascending; the knots of jrange[b] ascending; then ((C' + sum M' E) + sum M dE) / (double)N, N the
// caller's fp32 number, rounded to fp32 once at the store. An absent input group is the value 0.0 in the same arithmetic,
// with its loads (and, without d_tau and dTs, both Planck evaluations) left out: the same bits as zeros passed. No atomics.
// A value of dL depends on its own vector, temperature and band alone: the same bits run to run, for a vector or a
// temperature alone or among others, for any subset of the bands (order kept).
#include "rtx_srf_common.h"
#include "rtx_tud_jac_common.h"  // planck_dT

#define SRFJ_NV 4                       // tangent vectors per call: rtx_srf_radiance_jvp_max_vectors()
#define SRFJ_MAXT 2                     // temperatures per call: rtx_srf_radiance_jvp_max_temps()
#define SRFJ_NQ (SRFJ_NV * SRFJ_MAXT)   // m' of a point: SRFJ_NQ fp64 numbers, 64 KiB of LDS for the chunk
#define SRFJ_SUB 64                     // points per sub-chunk, as rtx_srf_moments'
#define SRFJ_NSUB (SRF_CH / SRFJ_SUB)
#define SRFJ_WAVES (SRF_CH / 64)

struct SrfjArgs {
  SrfArgs s;  // g, nx, kx, kr, ng, ks, sup as in rtx_srf_moments; X = NULL (uniform grid), the rest unused
  const float *tau, *Ld;
  const float *d_tau, *d_La, *d_Ld;  // [nv][ld_d] each, or NULL
  long long ld_d;
  const double* dTs;                 // [nv][nT] on the device (library-owned staging), or NULL
  const double* Xk;
  long long nk, nE;
  int nT, nB, nv;
  int g0;                            // the launch group's first band
  int pts;                           // C' and M' are formed (a row or dTs is given)
  double ct[SRFJ_MAXT];              // 100 c2 log2(e) / Ts_t
  long long row;                     // elements per workspace row: nk + 2 * (sub-chunks of the grid)
  double* WC;                        // [n_chunks][SRF_SLOTS][SRFJ_NV] chunk sums of w c'
  double* P;                         // [SRF_SLOTS][nv][nT][row] sub-chunk sums of w m' hat
  double* Cp;                        // [nv][nB]
  double* Mp;                        // [nv][nT][nB][nk]
  const float *N, *M, *E, *dE;
  const int2* jrange;
  float* dL;
};

__global__ __launch_bounds__(64) void srfj_support_kernel(SrfjArgs a) {
  const int j = threadIdx.x;
  if (j >= a.s.ng) return;
  const double x_first = a.s.kx[a.s.ks[j]], x_last = a.s.kx[a.s.ks[j + 1] - 1];
  a.s.sup[2 * j] = srf_bound(a.s, x_first, 0);
  a.s.sup[2 * j + 1] = srf_bound(a.s, x_last, 1);
}

__global__ __launch_bounds__(SRF_CH) void srfj_chunk_kernel(SrfjArgs a) {
  const long long chunk = blockIdx.x;
  const long long r0 = chunk * SRF_CH, r1 = r0 + SRF_CH < a.s.nx ? r0 + SRF_CH : a.s.nx;
  const int np = (int)(r1 - r0);  // points of this chunk
  const int p = threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nq = a.nv * a.nT;
  __shared__ double s_m[SRF_CH * SRFJ_NQ];  // m' of point i, vector v, temperature t: element (i nv + v) nT + t
  __shared__ double s_c[SRF_CH * SRFJ_NV];  // c' of point i, vector v: element i nv + v
  __shared__ float2 s_h[SRF_CH];            // the point's weights on knots j0 and j0 + 1 (srfm_hats; (1, 0) outside the knots)
  __shared__ int s_j0[SRF_CH];              // its lower knot; past the grid's end: INT_MAX
  __shared__ float s_w[SRF_CH];             // one band's weights
  __shared__ double s_kx[SRF_MAX_KNOTS];    // one band's knots under the chunk
  __shared__ float s_kr[SRF_MAX_KNOTS];
  __shared__ int s_lo[SRF_SLOTS], s_hi[SRF_SLOTS];  // support of band j within the chunk as rows [lo, hi) from r0
  __shared__ int s_ja[SRFJ_NSUB], s_kn[SRFJ_NSUB], s_koff[SRFJ_NSUB + 1];  // first knot, knots and task offset of a sub-chunk
  __shared__ double s_red[SRFJ_NV][SRFJ_WAVES];
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
  int ua = SRF_CH, ub = 0;  // rows under any band of the group: only they are read and evaluated
  for (int j = 0; j < SRF_SLOTS; ++j)
    if (s_hi[j] > s_lo[j]) { ua = min(ua, s_lo[j]); ub = max(ub, s_hi[j]); }
  // ---- the chunk's points: the knot interval as srfm_chunk_kernel forms it, then c' and m' of every vector
  double x = 0.0;
  {
    int j0 = 0x7fffffff;
    float h0 = 1.f, h1 = 0.f;
    if (p < np) {
      const long long i = r0 + p;
      x = srf_x(a.s, i);
      const long long cnt = srfm_count(a.Xk, a.nk, x);
      j0 = (int)(cnt > 0 ? cnt - 1 : 0);
      if (cnt > 0 && cnt < a.nk) srfm_hats(x, a.Xk[cnt - 1], a.Xk[cnt], h0, h1);
      if (p >= ua && p < ub) {  // elsewhere every band's weight is 0 and c', m' are never read
        const double tt = (double)a.tau[i], ld = (double)a.Ld[i];
        double dt[SRFJ_NV], dd[SRFJ_NV];
#pragma unroll
        for (int v = 0; v < SRFJ_NV; ++v) {
          dt[v] = dd[v] = 0.0;
          if (v < a.nv) {
            const size_t e = (size_t)v * (size_t)a.ld_d + (size_t)i;
            dt[v] = a.d_tau ? (double)a.d_tau[e] : 0.0;
            dd[v] = a.d_Ld ? (double)a.d_Ld[e] : 0.0;
            const double da = a.d_La ? (double)a.d_La[e] : 0.0;
            s_c[p * a.nv + v] = (dt[v] * ld + tt * dd[v]) + da;
          }
        }
        const bool planck = a.d_tau || a.dTs;  // uniform
        const double x100 = x * 100.0;
        const double c1x3 = RT_C1 * (x100 * x100 * x100) * 1e4;
        for (int t = 0; t < a.nT; ++t) {
          float B = 0.f, dB = 0.f;
          if (planck) planck_dT(c1x3, x, a.ct[t], B, dB);
          const double bl = (double)B - ld;
#pragma unroll
          for (int v = 0; v < SRFJ_NV; ++v) {
            if (v < a.nv) {
              const double ts = a.dTs ? a.dTs[v * a.nT + t] : 0.0;
              s_m[(p * a.nv + v) * a.nT + t] = dt[v] * bl + tt * ((double)dB * ts - dd[v]);
            }
          }
        }
      }
    }
    s_j0[p] = j0; s_h[p] = make_float2(h0, h1);
  }
  __syncthreads();
  if (threadIdx.x < SRFJ_NSUB) {  // the knots a sub-chunk touches: lower knot of its first point .. upper knot of its last
    const int first = SRFJ_SUB * threadIdx.x, last = min(first + SRFJ_SUB, np) - 1;
    int ja = 0, kn = 0;
    if (first < np) {
      ja = s_j0[first];
      const long long jb = min((long long)s_j0[last] + 1, a.nk - 1);
      kn = (int)(jb - ja + 1);
    }
    s_ja[threadIdx.x] = ja; s_kn[threadIdx.x] = kn;
  }
  __syncthreads();
  if (threadIdx.x <= SRFJ_NSUB) {
    int off = 0;
    for (int s = 0; s < (int)threadIdx.x; ++s) off += s_kn[s];
    s_koff[threadIdx.x] = off;
  }
  __syncthreads();
  const long long ntask = (long long)s_koff[SRFJ_NSUB] * nq;
  for (int j = 0; j < a.s.ng; ++j) {
    const int lo = s_lo[j], hi = s_hi[j];
    if (hi <= lo) continue;  // uniform over the workgroup
    // ---- the band's weights: srf_weight on the knots under the chunk, the segment found as srfv_point_kernel finds it
    float w = 0.f;
    {
      const double* kx = a.s.kx + a.s.ks[j];
      const int nkb = a.s.ks[j + 1] - a.s.ks[j];
      const int jA = srf_segment(kx, nkb, srf_x(a.s, r0 + lo));
      const int m = srf_segment(kx, nkb, srf_x(a.s, r0 + hi - 1)) + 2 - jA;  // knots jA .. jB + 1
      for (int q = threadIdx.x; q < m; q += SRF_CH) { s_kx[q] = kx[jA + q]; s_kr[q] = a.s.kr[a.s.ks[j] + jA + q]; }
      __syncthreads();
      if (p >= lo && p < hi) {
        int u = 1, v = m - 1;  // the segment srf_weight's walk from 0 would reach: the knots 1 .. m - 2 that are <= x
        while (u < v) {
          const int mid = (u + v) >> 1;
          if (x >= s_kx[mid]) u = mid + 1; else v = mid;
        }
        int seg = u - 1;
        w = srf_weight(a.s, s_kx, s_kr, m, seg, r0 + p);
      }
      s_w[p] = w;
    }
    // ---- the chunk's sums of w c': the lanes of a wave, then the waves in order
#pragma unroll
    for (int v = 0; v < SRFJ_NV; ++v) {
      if (v < a.nv) {  // uniform
        double c = w != 0.f ? (double)w * s_c[p * a.nv + v] : 0.0;  // a row of weight 0 is skipped, not multiplied
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
        if (lane == 0) s_red[v][wave] = c;
      }
    }
    __syncthreads();  // s_w and s_red are written
    if (p < a.nv) {
      double c = 0.0;
      for (int q = 0; q < SRFJ_WAVES; ++q) c += s_red[p][q];
      a.WC[((size_t)chunk * SRF_SLOTS + j) * SRFJ_NV + p] = c;
    }
    // ---- knot sums: task = (sub-chunk, knot it touches, vector, temperature), temperature fastest
    for (long long task = threadIdx.x; task < ntask; task += SRF_CH) {
      const int q = (int)(task % nq), kk = (int)(task / nq);
      int s = 0;
      while (kk >= s_koff[s + 1]) ++s;
      const int b0 = max(SRFJ_SUB * s, lo), b1 = min(SRFJ_SUB * (s + 1), hi);
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
      double acc = 0.0;
      for (int i = u; i < e; ++i) {
        const float wi = s_w[i];
        const float2 h = s_h[i];
        const float hat = s_j0[i] == jk ? h.x : h.y;
        if (wi != 0.f) acc += ((double)wi * s_m[i * nq + q]) * (double)hat;  // a row of weight 0 is skipped
      }
      a.P[((size_t)j * nq + q) * (size_t)a.row + (size_t)jk + 2 * (size_t)(chunk * SRFJ_NSUB + s)] = acc;
    }
    __syncthreads();  // s_w, the knots and s_red are rewritten by the next band
  }
}

// one thread per (vector, temperature, knot) of a band: the knot's sub-chunk sums in ascending order, as
// srfm_reduce_kernel finds them; the first nv threads of a band also add its chunk sums of w c'
__global__ __launch_bounds__(256) void srfj_reduce_kernel(SrfjArgs a) {
  const int j = blockIdx.x, b = a.g0 + j;
  const int nq = a.nv * a.nT;
  const long long q = (long long)blockIdx.y * 256 + threadIdx.x;
  const long long lo = a.s.sup[2 * j], hi = a.s.sup[2 * j + 1];
  if (q < a.nk * nq) {
    const int qq = (int)(q / a.nk);
    const long long jk = q - (long long)qq * a.nk;
    const int2 jr = a.jrange[b];
    double acc = 0.0;
    if (hi > lo && jk >= jr.x && jk <= jr.y) {
      long long sA = lo / SRFJ_SUB, sB = (hi - 1) / SRFJ_SUB;
      if (jk >= 2) sA = max(sA, srf_bound(a.s, a.Xk[jk - 1], 0) / SRFJ_SUB);
      if (jk <= a.nk - 2) {
        const long long pp = srf_bound(a.s, a.Xk[jk + 1], 0);  // rows from pp on lie in interval jk + 1 or above
        sB = pp > 0 ? min(sB, (pp - 1) / SRFJ_SUB) : -1;
      }
      const double* row = a.P + ((size_t)j * nq + qq) * (size_t)a.row + (size_t)jk;
      for (long long s = sA; s <= sB; ++s) acc += row[2 * s];
    }
    a.Mp[((size_t)qq * a.nB + b) * (size_t)a.nk + jk] = acc;  // 0 on the knots the band does not touch
  }
  if (blockIdx.y == 0 && threadIdx.x < a.nv) {
    double C = 0.0;
    if (hi > lo)
      for (long long ch = lo / SRF_CH; ch <= (hi - 1) / SRF_CH; ++ch) C += a.WC[((size_t)ch * SRF_SLOTS + j) * SRFJ_NV + threadIdx.x];
    a.Cp[(size_t)threadIdx.x * a.nB + b] = C;
  }
}

// one thread per (band, column, vector and temperature): the three terms in the order written, over jrange[b] ascending
__global__ __launch_bounds__(256) void srfj_mix_kernel(SrfjArgs a) {
  const int b = blockIdx.x, qq = blockIdx.z;
  const long long e = (long long)blockIdx.y * 256 + threadIdx.x;
  if (e >= a.nE) return;
  const int v = qq / a.nT, t = qq - v * a.nT;
  const int2 jr = a.jrange[b];
  const long long ja = jr.x > 0 ? jr.x : 0, jb = jr.y < a.nk - 1 ? jr.y : a.nk - 1;  // a range that is not the forward's reads nothing outside
  double c = 0.0, s1 = 0.0, s2 = 0.0;
  if (a.pts) {
    c = a.Cp[(size_t)v * a.nB + b];
    const double* Mp = a.Mp + ((size_t)qq * a.nB + b) * (size_t)a.nk;
    for (long long j = ja; j <= jb; ++j) s1 += Mp[j] * (double)a.E[(size_t)j * a.nE + e];
  }
  if (a.dE) {
    const float* M = a.M + ((size_t)t * a.nB + b) * (size_t)a.nk;
    const float* dE = a.dE + (size_t)v * (size_t)a.nk * (size_t)a.nE;
    for (long long j = ja; j <= jb; ++j) s2 += (double)M[j] * (double)dE[(size_t)j * a.nE + e];
  }
  // N = 0: no point under the band, every sum is 0 and 0 / 0 = NaN, as the band's L
  a.dL[(((size_t)v * a.nT + t) * a.nB + b) * (size_t)a.nE + e] = (float)(((c + s1) + s2) / (double)a.N[b]);
}

// workspace and the staged dTs, per (device, stream)
static StreamScratch* const srfj_scratch = new StreamScratch();
static StreamScratch* const srfj_stage = new StreamScratch();

extern "C" int rtx_srf_radiance_jvp_max_vectors(void) { return SRFJ_NV; }
extern "C" int rtx_srf_radiance_jvp_max_temps(void) { return SRFJ_MAXT; }

extern "C" int rtx_srf_radiance_jvp(const rtx_grid* grid, const float* tau, const float* Ld, const float* d_tau, const float* d_La,
                                    const float* d_Ld, int64_t ld_d, const double* Ts_h, const double* dTs_h, int nT,
                                    const double* Xk, int64_t nk, int nB, const int32_t* knot_start_h, const double* knot_x_d,
                                    const float* knot_r_d, const float* N, const float* M, const int32_t* jrange, const float* E,
                                    const float* dE, int64_t nE, int n_vec, float* dL, void* stream) {
  if (!grid) RTX_FAIL("no grid");
  if (rtx_check_grid(grid)) return 1;
  if (nk < 1) RTX_FAIL("nk=%lld: need at least 1 emissivity knot", (long long)nk);
  if (nk > (1ll << 23)) RTX_FAIL("nk=%lld: at most %lld emissivity knots", (long long)nk, 1ll << 23);
  if (nT < 1 || nT > SRFJ_MAXT) RTX_FAIL("nT=%d outside [1,%d] (rtx_srf_radiance_jvp_max_temps)", nT, SRFJ_MAXT);
  if (n_vec < 1 || n_vec > SRFJ_NV) RTX_FAIL("n_vec=%d outside [1,%d] (rtx_srf_radiance_jvp_max_vectors)", n_vec, SRFJ_NV);
  if (nE < 1) RTX_FAIL("nE=%lld: need at least 1 emissivity column", (long long)nE);
  if (nB < 0) RTX_FAIL("negative size");
  if (!d_tau && !d_La && !d_Ld && !dTs_h && !dE) RTX_FAIL("no tangent: d_tau, d_La, d_Ld, dTs_h and dE are all NULL");
  if (nB == 0) return 0;
  if (!tau || !Ld || !Ts_h || !Xk || !knot_start_h || !knot_x_d || !knot_r_d || !N || !M || !jrange || !E || !dL)
    RTX_FAIL("a required pointer is NULL");
  const long long nx = grid->n;
  if ((d_tau || d_La || d_Ld) && ld_d < nx) RTX_FAIL("ld_d=%lld < grid->n=%lld", (long long)ld_d, nx);
  for (int t = 0; t < nT; ++t)
    if (!(Ts_h[t] > 0.0)) RTX_FAIL("surface temperature %g", Ts_h[t]);
  if (dTs_h)
    for (int q = 0; q < n_vec * nT; ++q)
      if (!isfinite(dTs_h[q])) RTX_FAIL("dTs_h[%d] is not finite", q);
  if (knot_start_h[0] < 0) RTX_FAIL("knot_start[0]=%d is negative", (int)knot_start_h[0]);
  for (int b = 0; b < nB; ++b) {
    const long long n = (long long)knot_start_h[b + 1] - (long long)knot_start_h[b];
    if (n < 0) RTX_FAIL("knot_start is not ascending at band %d", b);
    if (n < 2) RTX_FAIL("band %d has %lld knots: a response table needs at least 2", b, n);
    if (n > SRF_MAX_KNOTS) RTX_FAIL("band %d has %lld knots: at most %d", b, n, SRF_MAX_KNOTS);
  }
  const long long n_chunks = (nx + SRF_CH - 1) / SRF_CH;
  if (n_chunks > 0x7fffffffLL / SRFJ_NSUB) RTX_FAIL("grid->n=%lld: too many chunks", nx);
  const int nq = n_vec * nT;
  const long long nqb = ((long long)nk * nq + 255) / 256;  // blocks of the reduce kernel per band
  if (nqb > 65535) RTX_FAIL("nk=%lld x n_vec=%d x nT=%d: too many for one call", (long long)nk, n_vec, nT);
  const long long neb = ((long long)nE + 255) / 256;
  if (neb > 65535) RTX_FAIL("nE=%lld: too many columns for one call", (long long)nE);
  hipStream_t st = (hipStream_t)stream;
  SrfjArgs a;
  memset(&a, 0, sizeof(a));
  a.pts = d_tau || d_La || d_Ld || dTs_h;
  a.row = (long long)nk + 2 * n_chunks * SRFJ_NSUB;
  const size_t nW = a.pts ? (size_t)n_chunks * SRF_SLOTS * SRFJ_NV : 0, nP = a.pts ? (size_t)SRF_SLOTS * (size_t)nq * (size_t)a.row : 0,
               nC = a.pts ? (size_t)n_vec * (size_t)nB : 0, nM = a.pts ? (size_t)nq * (size_t)nB * (size_t)nk : 0;
  char* base = nullptr;
  if (srfj_scratch->get(st, (nW + nP + nC + nM) * sizeof(double) + 2 * SRF_SLOTS * sizeof(long long), (void**)&base)) return 1;
  a.WC = (double*)base; a.P = a.WC + nW; a.Cp = a.P + nP; a.Mp = a.Cp + nC; a.s.sup = (long long*)(a.Mp + nM);
  if (dTs_h) {
    void* d = nullptr;
    if (srfj_stage->get(st, (size_t)nq * sizeof(double), &d)) return 1;
    RTX_HIP(hipMemcpyAsync(d, dTs_h, (size_t)nq * sizeof(double), hipMemcpyHostToDevice, st));  // pageable: staged before returning
    a.dTs = (const double*)d;
  }
  a.s.g = to_dev(grid);
  a.s.nx = nx; a.s.kx = knot_x_d; a.s.kr = knot_r_d;
  a.tau = tau; a.Ld = Ld; a.d_tau = d_tau; a.d_La = d_La; a.d_Ld = d_Ld; a.ld_d = ld_d;
  a.Xk = Xk; a.nk = nk; a.nE = nE; a.nT = nT; a.nB = nB; a.nv = n_vec;
  for (int t = 0; t < SRFJ_MAXT; ++t) a.ct[t] = t < nT ? c2l2e_over(Ts_h[t]) : 0.0;
  a.N = N; a.M = M; a.E = E; a.dE = dE; a.jrange = reinterpret_cast<const int2*>(jrange); a.dL = dL;
  if (a.pts) {
    for (int g0 = 0; g0 < nB; g0 += SRF_SLOTS) {
      a.g0 = g0;
      a.s.ng = nB - g0 < SRF_SLOTS ? nB - g0 : SRF_SLOTS;
      for (int j = 0; j <= SRF_SLOTS; ++j) a.s.ks[j] = knot_start_h[g0 + (j < a.s.ng ? j : a.s.ng)];
      hipLaunchKernelGGL(srfj_support_kernel, dim3(1), dim3(64), 0, st, a);
      RTX_LAUNCH_CHECK();
      if (n_chunks > 0) {
        hipLaunchKernelGGL(srfj_chunk_kernel, dim3((unsigned)n_chunks), dim3(SRF_CH), 0, st, a);
        RTX_LAUNCH_CHECK();
      }
      hipLaunchKernelGGL(srfj_reduce_kernel, dim3((unsigned)a.s.ng, (unsigned)nqb), dim3(256), 0, st, a);
      RTX_LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL(srfj_mix_kernel, dim3((unsigned)nB, (unsigned)neb, (unsigned)nq), dim3(256), 0, st, a);
  RTX_LAUNCH_CHECK();
  return 0;
}
