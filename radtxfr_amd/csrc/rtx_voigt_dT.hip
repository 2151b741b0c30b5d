// Analytic temperature derivative of the Voigt line-sum on a uniform grid: rtx_voigt_sum_dt, after
// rtx_line_prep_dt (rtx_lines.hip), writes d OD / dT per layer with every line's window held fixed.
//
// Per line and point, g = A K(x, y), K + iL = hum1_wei(x, y) (misc/hapi.py:9833-9844), and
//   dg/dT = A [alpha K + K_x x' + K_y y'],   x' = -sx - x h,   y' = gy - y h      (records: rtx_common.h)
//   |x| + y < 15 (Weideman-24):  K_x = -2 (x K - y L),  K_y = 2 (x L + y K) - 2/sqrt(pi)       [w' = -2 z w + 2i/sqrt(pi)]
//   elsewhere, t = y - ix, w = t / (sqrt(pi) (1/2 + t^2)):  K_y + i K_x = dw/dt = (1/2 - t^2) / (sqrt(pi) (1/2 + t^2)^2)
// A point takes the derivative of its own branch; the jump of hum1_wei at the switch is not differentiated.
//
// The scheme is voigt_scatter_kernel's (rtx_voigt_scatter.hip): one workgroup per tile of 1024 points and layer; the
// candidates of the tile's canonical range are dealt to the four waves in table order, EACH LINE IS TAKEN BY EXACTLY ONE
// WAVE, which adds it into its own copy of the tile in LDS (plain read / add / write); rows of 64 points are a run-time
// loop, masked only where a window edge cuts them; the four copies are added in a fixed order. No atomics: two calls give
// the same bits, and a tile-aligned shard gives the bits of the full grid. Every point is evaluated directly.
//
// Precision. Far rows and the far lanes of band rows: the rational above in fp32, about 20 VALU + one v_rcp_f32, no
// cancellation (see far_dT). Band lanes (|x| + y < 15): fp64 for every line, not only y < 1 ones. K_y is the small
// difference 2 (x L + y K) - 2/sqrt(pi) ~ 1/(sqrt(pi) x^2), 2e-3 of its terms at |x| = 15; the fp32 Weideman value is within
// 1.8e-6 (absolute) of w, which leaves 2 |x| 1.8e-6 = 5e-5 in a K_y of 2.5e-3: 2 % of the term, far above the 5e-5 the
// tests allow. In fp64 the same difference keeps 12 digits. Band rows are the 2-3 rows around a line's centre.
#include "rtx_common.h"

#include "rtx_voigt_math.h"

#define DT_ROWS 16  // rows of 64 points per tile: the tile of rtx_voigt_tile_points(), whose candidate ranges this kernel reads

struct DtArgs {
  const LineRec* rec;
  const LineRec64* rec64;
  const LineRecDT* drec;
  const LineRecDT64* drec64;
  const int2* ranges;
  long long n_lines;
  int n_tiles;
  GridDev g;
  float* out32;
  double* out64;
  long long ld;
  double inv_scale;
};

// The far-wing derivative of one line at u = i - i0 (an exact integer-valued float). With p = yh - xx, q = 2 x y and
// R = p^2 + q^2 = (xx + b1) xx + b0:  sqrt(pi) K = y (yh + xx) / R,  sqrt(pi) K_x = q (2p/R - 1) / R,
// sqrt(pi) K_y = ((p^2 - q^2)/R - p) / R. Every factor is formed from terms of one sign or of different size (far from the
// centre p ~ -xx and (p^2 - q^2)/R ~ 1 against -p ~ xx); dividing by R once per factor keeps x^8 out of the fp32 range.
// ay = alpha y, hoisted per line.
__device__ __forceinline__ float far_dT(float u, const LineRec& q, const LineRecDT& d, float ay) {
  const float x = fmaf(u, q.a, q.c);
  const float xx = x * x;
  const float rR = __builtin_amdgcn_rcpf(fmaf(xx + q.b1, xx, q.b0));
  const float p = d.yh - xx;
  const float qq = d.y2 * x;
  const float xp = -fmaf(x, d.h, d.sx);
  const float kx = qq * fmaf(2.0f * p, rR, -1.0f);
  const float ky = fmaf(fmaf(p, p, -(qq * qq)), rR, -p);
  return (d.Ap * rR) * fmaf(ky, d.yp, fmaf(kx, xp, ay * (d.yh + xx)));
}

// One band row: the lanes inside |x| + y < 15 -- the reference's switch, formed in fp64 exactly as it forms it, x = -Im Z1
// = -((sg0 - sg) cte) -- take the Weideman branch in fp64; the others keep the far-wing value. Lanes outside [ulo, uhi) add 0.
__device__ __forceinline__ float band_dT(const DtArgs& a, const LineRec64& Q, const LineRecDT64& D, const LineRec& q, const LineRecDT& d,
                                         float ay, float u, int i, float ulo, float uhi) {
  float v = far_dT(u, q, d, ay);
  const double sg = grid_x(a.g, a.g.offset + (long long)i);
  const double x = -((Q.sg0 - sg) * Q.cte);
  if (fabs(x) + Q.y < 15.0) {
    double K, L;
    weideman_cplx<double>(x, Q.y, K, L);
    const double Kx = -2.0 * fma(x, K, -(Q.y * L));
    const double Ky = fma(2.0, fma(x, L, Q.y * K), -2.0 * INV_SQRT_PI);
    const double xp = -fma(x, D.h, D.sx);
    const double yp = fma(-Q.y, D.h, D.gy);
    v = (float)(Q.A * fma(Ky, yp, fma(Kx, xp, D.alpha * K)));
  }
  return (u >= ulo && u < uhi) ? v : 0.f;
}

// One line, taken by one wave: its rows of the tile into the wave's LDS copy. The records arrive through scalar loads.
__device__ __forceinline__ void visit_line_dT(const DtArgs& a, const LineRec* __restrict__ rec, const LineRec64* __restrict__ rec64,
                                              const LineRecDT* __restrict__ drec, const LineRecDT64* __restrict__ drec64, int slot,
                                              float* __restrict__ acc, int ia, int ib, int nt, int lane, float lanef) {
  const LineRec q = rec[slot];
  const int qi0 = __builtin_amdgcn_readfirstlane(q.i0), qlo = __builtin_amdgcn_readfirstlane(q.lo);
  const int qhi = __builtin_amdgcn_readfirstlane(q.hi), qzw = __builtin_amdgcn_readfirstlane(q.zw);
  if (!(qhi > ia && qlo < ib)) return;  // empty windows have lo = hi = 0
  const LineRecDT d = drec[slot];
  const float ay = d.alpha * d.y;
  // row geometry, tile-local, in plain integer arithmetic (row_geom of rtx_voigt_scatter.hip without the near zone)
  const int dlo = qlo - ia, dhi = qhi - ia;
  const int lo_t = dlo > 0 ? dlo : 0, hi_t = dhi < nt ? dhi : nt;
  const int r_lo = lo_t >> 6, r_hi = (hi_t + 63) >> 6;  // rows the window reaches: r_hi <= DT_ROWS since hi_t <= nt <= 64 DT_ROWS
  const int c0 = (lo_t + 63) >> 6;                      // rows wholly inside the window: [c0, c1)
  const int c1 = dhi < nt ? hi_t >> 6 : r_hi;           // a ragged last row of the GRID is not an edge: its stores are masked
  int z0 = DT_ROWS, z1 = -1;                            // rows touching the band |i - i0| <= zw: [z0, z1]
  if (qzw > 0) {
    const int zl = qi0 - qzw - ia, zh = qi0 + qzw - ia;  // |qi0| <= 1e8 + n, zw <= 4e7 (prologue clamps): no overflow
    if (zh >= 0 && zl < 64 * DT_ROWS) {
      z0 = zl > 0 ? zl >> 6 : 0;
      z1 = (zh >> 6) < DT_ROWS - 1 ? zh >> 6 : DT_ROWS - 1;
    }
  }
  const float u0 = (float)(ia - qi0) + lanef;  // exact while |i - i0| < 2^24
  const float ulo = (float)(qlo - qi0), uhi = (float)(qhi - qi0);

  // interior rows = [c0, c1) minus [z0, z1]: run 0 = [c0, min(c1, z0)), run 1 = [max(c0, z1 + 1), c1)
  for (int run = 0; run < 2; ++run) {
    if (run == 1 && z0 > z1) break;
    int r = run == 0 ? c0 : (z1 + 1 > c0 ? z1 + 1 : c0);
    const int re = run == 0 ? (z0 < c1 ? z0 : c1) : c1;
    for (; r + 4 <= re; r += 4) {  // 4 rows in flight: LDS reads, 4 evaluations, LDS writes
      float* p = acc + r * 64 + lane;
      const float a0 = p[0], a1 = p[64], a2 = p[128], a3 = p[192];
      const float ub = u0 + (float)(64 * r);
      p[0] = a0 + far_dT(ub, q, d, ay);
      p[64] = a1 + far_dT(ub + 64.0f, q, d, ay);
      p[128] = a2 + far_dT(ub + 128.0f, q, d, ay);
      p[192] = a3 + far_dT(ub + 192.0f, q, d, ay);
    }
    for (; r < re; ++r) {
      float* p = acc + r * 64 + lane;
      p[0] += far_dT(u0 + (float)(64 * r), q, d, ay);
    }
  }
  // the rows a window edge cuts (at most two) outside the band rows: far-wing form, lanes outside [lo, hi) masked
  const int eL = c0 != r_lo ? r_lo : -1;
  const int eR = (c1 != r_hi && r_hi - 1 != eL) ? r_hi - 1 : -1;
  for (int pass = 0; pass < 2; ++pass) {
    const int r = pass == 0 ? eL : eR;
    if (r < 0 || (r >= z0 && r <= z1)) continue;
    float* p = acc + r * 64 + lane;
    const float u = u0 + (float)(64 * r);
    const float v = far_dT(u, q, d, ay);
    p[0] += (u >= ulo && u < uhi) ? v : 0.f;
  }
  if (z0 <= z1) {
    const int zb = z0 > r_lo ? z0 : r_lo, ze = z1 < r_hi - 1 ? z1 : r_hi - 1;
    if (zb <= ze) {
      const LineRec64 Q = rec64[slot];
      const LineRecDT64 D = drec64[slot];
      for (int r = zb; r <= ze; ++r) {
        float* p = acc + r * 64 + lane;
        p[0] += band_dT(a, Q, D, q, d, ay, u0 + (float)(64 * r), ia + 64 * r + lane, ulo, uhi);
      }
    }
  }
}

__global__ __launch_bounds__(256) void voigt_dT_kernel(DtArgs a) {
  constexpr int TILE = 64 * DT_ROWS;
  __shared__ float s_acc[4][TILE];  // one private tile per wave
  const int k = blockIdx.y;
  const int tile = xcd_tile(blockIdx.x);  // XCD-aware order (rtx_common.h)
  if (tile >= a.n_tiles) return;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const long long n = a.g.n;
  const int ia = tile * TILE;
  const int ib = (int)((long long)ia + TILE < n ? (long long)ia + TILE : n);
  const int nt = ib - ia;
  const size_t ko = (size_t)k * (size_t)a.n_lines;
  const int2 rng = a.ranges[(size_t)k * a.n_tiles + tile];
  float* __restrict__ acc = s_acc[wave];
#pragma unroll
  for (int r = 0; r < DT_ROWS; ++r) acc[r * 64 + lane] = 0.f;
  const float lanef = (float)lane;
  for (int slot = rng.x + wave; slot < rng.y; slot += 4)
    visit_line_dT(a, a.rec + ko, a.rec64 + ko, a.drec + ko, a.drec64 + ko, slot, acc, ia, ib, nt, lane, lanef);
  __syncthreads();  // every wave's tile is complete
  // fixed-order sum of the four copies, coalesced stores; the ragged last row of the grid is masked here
#pragma unroll 4
  for (int r = wave; r < DT_ROWS; r += 4) {
    const int t = r * 64 + lane;
    const long long i = (long long)ia + t;
    const float v = (s_acc[0][t] + s_acc[1][t]) + (s_acc[2][t] + s_acc[3][t]);
    if (i < (long long)ib) {
      const size_t o = (size_t)k * (size_t)a.ld + (size_t)i;
      if (a.out32) a.out32[o] = v;
      if (a.out64) a.out64[o] = (double)v * a.inv_scale;
    }
  }
}

// rtx_voigt.hip
extern "C" int rtx_voigt_tile_points(void);
void rtx_launch_tile_ranges_n(const rtx_prep* P, long long n, int n_layers, int n_tiles, int tile, hipStream_t st);

extern "C" int rtx_voigt_sum_dt(const rtx_prep* P, const rtx_grid* grid, int n_layers, float* out_f32, double* out_f64, int64_t ld,
                                void* stream) {
  if (!P) RTX_FAIL("prep is NULL");
  if (!P->dT) RTX_FAIL("the last prologue on this prep object was not rtx_line_prep_dt");
  if (rtx_check_grid(grid)) return 1;
  if (n_layers < 1 || n_layers != P->n_layers) RTX_FAIL("n_layers=%d does not match the last rtx_line_prep_dt (%d)", n_layers, P->n_layers);
  if (!out_f32 && !out_f64) RTX_FAIL("both outputs are NULL");
  if (ld < grid->n) RTX_FAIL("ld=%lld < n=%lld", (long long)ld, (long long)grid->n);
  if (grid->n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (P->n_lines == 0) {
    if (out_f32) RTX_HIP(hipMemset2DAsync(out_f32, ld * sizeof(float), 0, grid->n * sizeof(float), n_layers, st));
    if (out_f64) RTX_HIP(hipMemset2DAsync(out_f64, ld * sizeof(double), 0, grid->n * sizeof(double), n_layers, st));
    return 0;
  }
  constexpr int TILE = 64 * DT_ROWS;
  if (TILE != rtx_voigt_tile_points()) RTX_FAIL("rtx_voigt_sum_dt: tile of %d points, the prep object's is %d", TILE, rtx_voigt_tile_points());
  const long long n_tiles_ll = (grid->n + TILE - 1) / TILE;
  if (n_tiles_ll > P->max_tiles) RTX_FAIL("grid shard of %lld points exceeds the prep capacity", (long long)grid->n);
  const int n_tiles = (int)n_tiles_ll;
  rtx_launch_tile_ranges_n(P, grid->n, n_layers, n_tiles, TILE, st);  // canonical candidate ranges, no tile cut
  RTX_LAUNCH_CHECK();
  DtArgs a;
  a.rec = P->rec.get(); a.rec64 = P->rec64.get(); a.drec = P->drec.get(); a.drec64 = P->drec64.get();
  a.ranges = P->ranges.get(); a.n_lines = P->n_lines; a.n_tiles = n_tiles;
  a.g = to_dev(grid);
  a.out32 = out_f32; a.out64 = out_f64; a.ld = ld; a.inv_scale = 1.0 / P->scale;
  hipLaunchKernelGGL(voigt_dT_kernel, dim3(8 * xcd_slots(n_tiles), n_layers), dim3(256), 0, st, a);
  RTX_LAUNCH_CHECK();
  return 0;
}
