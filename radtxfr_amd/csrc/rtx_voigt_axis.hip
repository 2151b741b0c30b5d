// Voigt / Lorentz / Doppler line-sum on an explicit, possibly non-uniform axis (rtx_voigt_sum_axis, after
// rtx_line_prep_axis): what hapi.absorptionCoefficient_* compute on an OmegaGrid that is not an np.linspace (the reference
// sorts the grid and bisects it, misc/hapi.py:10979-10983, 11133-11134).
//
// The deterministic scheme of voigt_scatter_kernel (rtx_voigt_scatter.hip): a workgroup owns a tile of AX_TILE consecutive
// axis points of one layer; every candidate line of the tile's canonical range (tile_ranges_kernel on index-space inputs)
// is taken by exactly one wave, which accumulates it into its own copy of the tile in LDS; the four copies are added in a
// fixed order. No atomics: repeated calls give the same bits. Only the 64-point rows that meet a line's window [lo, hi) are
// visited, and the window is applied per point by index. Point by point everywhere (no Chebyshev-node far wings: on a
// non-uniform axis the nodes of a row are not fixed fractions of it). Hot tiles are not cut.
//
// Abscissa. With the tile's first point X[ia] as origin, d_i = X[i] - X[ia] is staged once per tile in LDS as two floats
// (d_i = dh_i + dl_i to 2^-48 relative), and per (line, tile) c = (X[ia] - sg0) * cte in fp64, split likewise, as is cte.
// Then x_i = c + d_i cte is formed as (dh*kh + ch) + (err(dh*kh) + cl + dh*kl + dl*kh), err() the exact product error by
// one fmaf: the result carries the rounding of x_i alone, like the uniform kernel's fmaf(u, a, c). The one-FMA form
// fmaf((float)d_i, (float)cte, (float)c) would carry an error of ~1e-7 of the tile span in x units, 1e-3 in x on a
// 0.02 cm^-1 tile of 1024 points (20 cm^-1 x cte ~ 600): 3e-5 of a pressure-broadened line's value next to its centre.
//
// Profile math: rtx_voigt_math.h, with the decisions of band_row: far-wing rational outside the Weideman band; in it,
// hum1_wei's switch |x|+y<15 (misc/hapi.py:9840) in fp32, redone in fp64 on x64 = -((sg0 - X[i]) * cte) -- formed as the
// reference forms it -- for lanes within 2e-3 of the switch; y >= 6 (or no band lane with |z| < 8) by the 6-term
// asymptotic series, else Weideman-24 in fp32; Doppler-dominated lines (y < 1) take fp64 Weideman on x64 on every band
// lane. Lorentz records carry y = 15 and no band: the far-wing rational is their exact profile.
#include <string.h>

#include "rtx_common.h"

#include "rtx_voigt_math.h"

#define AX_TILE 1024  // = rtx_voigt_tile_points() (checked at run time): the prep object's `ranges` capacity fits as it is
#define AX_ROWS (AX_TILE / 64)

struct AxisArgs {
  const LineRec* rec;
  const LineRec64* rec64;
  const int2* ranges;
  const double* X;
  long long n_lines;
  int n_tiles, nx;
  float* out32;
  double* out64;
  long long ld;
  double inv_scale;
};

// One line, taken by one wave: its rows of the tile, point by point, into the wave's LDS copy `acc`.
__device__ __forceinline__ void axis_line(const AxisArgs& a, const LineRec* __restrict__ rec, const LineRec64* __restrict__ rec64,
                                          int slot, float* __restrict__ acc, const float2* __restrict__ s_d, int ia, int ib,
                                          double xa, int lane) {
  const LineRec q = rec[slot];
  const int lo = __builtin_amdgcn_readfirstlane(q.lo), hi = __builtin_amdgcn_readfirstlane(q.hi);
  if (!(hi > ia && lo < ib)) return;  // empty windows have lo = hi = 0
  const int zlo = __builtin_amdgcn_readfirstlane(q.i0), zhi = __builtin_amdgcn_readfirstlane(q.zw);
  const LineRec64 Q = rec64[slot];
  const double c64 = (xa - Q.sg0) * Q.cte;  // x at X[ia]
  const float ch = (float)c64, cl = (float)(c64 - (double)ch);
  const float kh = (float)Q.cte, kl = (float)(Q.cte - (double)kh);
  const bool small_y = q.y < 1.0f;
  const int t_lo = lo > ia ? lo - ia : 0, t_hi = (hi < ib ? hi : ib) - ia;
  const int r_lo = t_lo >> 6, r_hi = (t_hi + 63) >> 6;
  for (int r = r_lo; r < r_hi; ++r) {
    const int t = r * 64 + lane;
    const int i = ia + t;
    const float2 d = s_d[t];
    const float p = d.x * kh;
    const float x = (p + ch) + fmaf(d.x, kl, fmaf(d.y, kh, cl + fmaf(d.x, kh, -p)));
    const float xx = x * x;
    float num = fmaf(xx, q.Ay, q.Ay0);
    float rden = __builtin_amdgcn_rcpf(fmaf(xx + q.b1, xx, q.b0));
    const int row0 = ia + 64 * r;
    if (row0 + 64 > zlo && row0 < zhi) {  // a row of the Weideman band (wave-uniform)
      const bool in_band = i >= zlo && i < zhi;  // [zlo, zhi) lies inside [lo, hi) and the axis
      if (small_y) {
        if (in_band) {
          const double x64 = -((Q.sg0 - a.X[i]) * Q.cte);
          if (fabs(x64) + Q.y < 15.0) {
            num = (float)(Q.A * weideman_re<double>(x64, Q.y));
            rden = 1.0f;
          }
        }
      } else {
        const float s32 = fabsf(x) + q.y;
        bool wz = in_band && s32 < 15.0f;
        const bool near = in_band && fabsf(s32 - 15.0f) < 2e-3f;
        if (__ballot(near) && near) {
          const double x64 = -((Q.sg0 - a.X[i]) * Q.cte);
          wz = fabs(x64) + Q.y < 15.0;
        }
        const bool series = q.y >= 6.0f || __ballot(wz && fmaf(x, x, q.y * q.y) < 64.0f) == 0ull;
        if (wz) {
          num = q.A * (series ? asym6_re(x, q.y) : weideman_re<float>(x, q.y));
          rden = 1.0f;
        }
      }
    }
    // the window, by index; lanes outside it (and past the axis) keep their sum untouched
    const float v = fmaf(num, rden, acc[t]);
    acc[t] = (i >= lo && i < hi) ? v : acc[t];
  }
}

__global__ __launch_bounds__(256) void voigt_axis_kernel(AxisArgs a) {
  __shared__ float s_acc[4][AX_TILE];  // one private tile per wave
  __shared__ float2 s_d[AX_TILE];      // X[ia + t] - X[ia] as two floats
  const int tile = blockIdx.x, k = blockIdx.y;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const int ia = tile * AX_TILE;
  const int ib = a.nx - ia < AX_TILE ? a.nx : ia + AX_TILE;
  const double xa = a.X[ia];
  for (int t = threadIdx.x; t < AX_TILE; t += 256) {
    float2 d = make_float2(0.f, 0.f);
    if (ia + t < ib) {
      const double dd = a.X[ia + t] - xa;
      d.x = (float)dd;
      d.y = (float)(dd - (double)d.x);
    }
    s_d[t] = d;
  }
  float* __restrict__ acc = s_acc[wave];
#pragma unroll
  for (int r = 0; r < AX_ROWS; ++r) acc[r * 64 + lane] = 0.f;
  __syncthreads();
  const LineRec* __restrict__ rec = a.rec + (size_t)k * (size_t)a.n_lines;
  const LineRec64* __restrict__ rec64 = a.rec64 + (size_t)k * (size_t)a.n_lines;
  const int2 rng = a.ranges[(size_t)k * a.n_tiles + tile];
  for (int slot = rng.x + wave; slot < rng.y; slot += 4) axis_line(a, rec, rec64, slot, acc, s_d, ia, ib, xa, lane);
  __syncthreads();  // every wave's tile is complete
  // fixed-order sum of the four copies, coalesced stores
  for (int r = wave; r < AX_ROWS; r += 4) {
    const int t = r * 64 + lane;
    const int i = ia + t;
    if (i < ib) {
      const float v = (s_acc[0][t] + s_acc[1][t]) + (s_acc[2][t] + s_acc[3][t]);
      const size_t o = (size_t)k * (size_t)a.ld + (size_t)i;
      if (a.out32) a.out32[o] = v;
      if (a.out64) a.out64[o] = (double)v * a.inv_scale;
    }
  }
}

// rtx_voigt.hip
void rtx_launch_tile_ranges_n(const rtx_prep* P, long long n, int n_layers, int n_tiles, int tile, hipStream_t st);

extern "C" int rtx_voigt_sum_axis(const rtx_prep* P, int n_layers, float* out_f32, double* out_f64, int64_t ld, void* stream) {
  if (!P) RTX_FAIL("prep is NULL");
  if (!P->axis) RTX_FAIL("rtx_voigt_sum_axis: the last prologue was not rtx_line_prep_axis");
  if (n_layers < 1 || n_layers != P->n_layers) RTX_FAIL("n_layers=%d does not match the last rtx_line_prep_axis (%d)", n_layers, P->n_layers);
  if (P->nx == 0) return 0;  // nothing to write
  if (!out_f32 && !out_f64) RTX_FAIL("both outputs are NULL");
  if (ld < P->nx) RTX_FAIL("ld=%lld < nx=%lld", (long long)ld, P->nx);
  if (rtx_voigt_tile_points() != AX_TILE) RTX_FAIL("line-sum tile of %d points, the axis kernel is built for %d", rtx_voigt_tile_points(), AX_TILE);
  hipStream_t st = (hipStream_t)stream;
  if (P->n_lines == 0) {
    if (out_f32) RTX_HIP(hipMemset2DAsync(out_f32, ld * sizeof(float), 0, P->nx * sizeof(float), n_layers, st));
    if (out_f64) RTX_HIP(hipMemset2DAsync(out_f64, ld * sizeof(double), 0, P->nx * sizeof(double), n_layers, st));
    return 0;
  }
  const int n_tiles = (int)((P->nx + AX_TILE - 1) / AX_TILE);  // <= max_tiles: the prologue checked nx against the capacity
  rtx_launch_tile_ranges_n(P, P->nx, n_layers, n_tiles, AX_TILE, st);
  RTX_LAUNCH_CHECK();
  AxisArgs a;
  a.rec = P->rec.get(); a.rec64 = P->rec64.get(); a.ranges = P->ranges.get(); a.X = P->X.get();
  a.n_lines = P->n_lines; a.n_tiles = n_tiles; a.nx = (int)P->nx;
  a.out32 = out_f32; a.out64 = out_f64; a.ld = ld; a.inv_scale = 1.0 / P->scale;
  hipLaunchKernelGGL(voigt_axis_kernel, dim3((unsigned)n_tiles, (unsigned)n_layers), dim3(256), 0, st, a);
  RTX_LAUNCH_CHECK();
  return 0;
}
