// Planck emission + Schwarzschild up/down-welling integration.
//
// rtx_planck : planckian(), reference radiative_transfer.py:792-848, fp64 like the reference.
// rtx_tud    : body of compute_TUD after the OD loop, radiative_transfer.py:340-392.
//
// TUD mapping (CDNA4): lane <-> wavenumber (coalesced dword loads of the layer-major OD), one point per lane, a
// run-time loop over the layers; OD is read from HBM exactly once and B is never materialised (the reference builds
// an (nX,nL) fp64 temporary, :340). Kernels, in the order the dispatcher prefers them:
//   tud_g_kernel        one (altitude, slant) pair: tau, L-up (bottom-up recurrence) and the downwelling as
//                       sum_k B_k [G(S_k) - G(S_k+1)], G = the angle-summed transmission function, tabulated in fp64
//   tud_g_snap_kernel   several altitudes / slants on an ascending height grid: one recurrence per slant, an altitude's
//                       outputs stored when the pass has done its count of layers
//   tud_g_pairs_kernel  the same for masks that are not prefixes: pairs in blocks of 3
//   tud_kernel<NA,COL>  the N_angle stream recurrences in registers (round 1's kernel): per-stream radiances
//                       (opts['save']) and the cross-check RADTXFR_TUD_KERNEL=streams
//
// Precision: exp arguments of the Planck term reach c2*nu/T ~ 40, where an fp32 argument alone
// costs 2.4e-6; the argument is formed in fp64, split into integer and fractional powers of two,
// and only the fractional part goes through v_exp_f32. Layer transmittances exp(-OD/cos) are
// fp32 (arguments matter only while OD < ~20).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>
#include <vector>

#include "rtx_tud_common.h"

// ---------------------------------------------------------------------------------------------------
struct PlanckArgs {
  GridDev g;
  const double* X;
  long long nx, nT;
  const double* T;
  int wavelength;
  double* out;
};

__global__ __launch_bounds__(256) void planck_kernel(PlanckArgs a) {
  const long long total = a.nx * a.nT;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long i = e / a.nT, j = e - i * a.nT;
    double X = a.X ? a.X[i] : grid_x(a.g, a.g.offset + i);
    const double T = a.T[j];
    double L;
    if (a.wavelength) {
      X = X * 1e-6;  // um -> m  (:839-841)
      L = RT_C1 / (pow(X, 5.0) * (exp(RT_C2 / (X * T)) - 1.0));
      L *= 1e-4;
    } else {
      X = X * 100.0;  // 1/cm -> 1/m  (:843-845)
      L = RT_C1 * (X * X * X) / (exp(RT_C2 * X / T) - 1.0);
      L *= 1e4;
    }
    a.out[e] = L;
  }
}

extern "C" int rtx_planck(const rtx_grid* grid, const double* X, int64_t nx, const double* T, int64_t nT, int wavelength,
                          double* out, void* stream) {
  if (!X) {
    if (rtx_check_grid(grid)) return 1;
    if (nx != grid->n) RTX_FAIL("nx=%lld != grid->n=%lld", (long long)nx, (long long)grid->n);
  }
  if (nx < 0 || nT < 0) RTX_FAIL("negative size");
  if (nx == 0 || nT == 0) return 0;
  if (!T || !out) RTX_FAIL("T/out is NULL");
  PlanckArgs a;
  if (grid) a.g = to_dev(grid); else { a.g.xmin = a.g.xmax = a.g.step = 0; a.g.n_total = a.g.offset = a.g.n = 0; }
  a.X = X; a.nx = nx; a.nT = nT; a.T = T; a.wavelength = wavelength; a.out = out;
  const long long total = nx * nT;
  long long blocks = (total + 255) / 256;
  if (blocks > 256 * 32) blocks = 256 * 32;
  hipLaunchKernelGGL(planck_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  RTX_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------
// Inverse Planck and its forward twin on brightness temperatures: brightnessTemperature()
// (radiative_transfer.py:851-933) and BT2L() (:936-1014). fp64, the reference's expressions and its
// bad-value masking (:922-923, :1004-1005). in/out are [nx][m], spectral axis first.
struct BtArgs {
  const double* X;
  long long nx, m;
  const double* in;
  int wavelength, inverse;  // inverse=1: radiance -> T ; 0: T -> radiance
  double bad;
  double* out;
};

__global__ __launch_bounds__(256) void bt_kernel(BtArgs a) {
  const long long total = a.nx * a.m;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long i = e / a.m;
    double X = a.X[i];
    const double v = a.in[e];
    double r;
    bool bad;
    if (a.inverse) {
      double L = v;
      if (a.wavelength) {
        X = X * 1e-6;  L = L * 1e4;   // (:913-915)
        r = RT_C2 / (X * log(1.0 + RT_C1 / (pow(X, 5.0) * L)));
      } else {
        X = X * 100.0;  L = L * 1e-4;  // (:917-919)
        r = RT_C2 * X / log(RT_C1 * (X * X * X) / L + 1.0);
      }
      bad = !isfinite(L) || (L <= 0.0);
    } else {
      const double T = v;
      if (a.wavelength) {
        X = X * 1e-6;  // (:995-997)
        r = RT_C1 / (pow(X, 5.0) * (exp(RT_C2 / (X * T)) - 1.0));
        r *= 1e-4;
      } else {
        X = X * 100.0;  // (:999-1001)
        r = RT_C1 * (X * X * X) / (exp(RT_C2 * X / T) - 1.0);
        r *= 1e4;
      }
      bad = !isfinite(r) || (T <= 0.0);
    }
    a.out[e] = bad ? a.bad : r;
  }
}

static int launch_bt(const double* X, int64_t nx, const double* in, int64_t m, int wavelength, int inverse, double bad,
                     double* out, void* stream) {
  if (nx < 0 || m < 0) RTX_FAIL("negative size");
  if (nx == 0 || m == 0) return 0;
  if (!X || !in || !out) RTX_FAIL("a required pointer is NULL");
  BtArgs a;
  a.X = X; a.nx = nx; a.m = m; a.in = in; a.wavelength = wavelength; a.inverse = inverse; a.bad = bad; a.out = out;
  long long blocks = (nx * m + 255) / 256;
  if (blocks > 256 * 32) blocks = 256 * 32;
  hipLaunchKernelGGL(bt_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  RTX_LAUNCH_CHECK();
  return 0;
}

extern "C" int rtx_brightness_temperature(const double* X, int64_t nx, const double* L, int64_t m, int wavelength,
                                          double bad_value, double* T_out, void* stream) {
  return launch_bt(X, nx, L, m, wavelength, 1, bad_value, T_out, stream);
}

extern "C" int rtx_bt2l(const double* X, int64_t nx, const double* T, int64_t m, int wavelength, double bad_value,
                        double* L_out, void* stream) {
  return launch_bt(X, nx, T, m, wavelength, 0, bad_value, L_out, stream);
}

// ---------------------------------------------------------------------------------------------------
#define TUD_MAX_LAYERS 128
#define TUD_MAX_ANGLES 128
#define TUD_MAX_ALT 16
#define TUD_MAX_MU 8

struct TudArgs {
  const float* OD;
  long long ld, ld_out;
  GridDev g;
  int n_layers, n_alt, n_mu, n_down, n_ang, return_od;
  float* tau;
  float* Lu;
  float* Ld;
  float* Ld_ang;                       // optional [n_ang_real][ld_out] per-stream radiances (opts['save'])
  int n_ang_real;
  float inv_wsum;                      // 1/sum(cos*sin) (inf/NaN propagate like the reference's 0/0)
  double c2l2e_over_T[TUD_MAX_LAYERS]; // 100*c2*log2(e)/T_k
  double c2l2e_over_Tmax, c2l2e_over_Tmin;  // the same for the warmest / coldest layer of the column
  float ang_c[TUD_MAX_ANGLES];         // -log2(e)/cos(theta)
  float ang_w[TUD_MAX_ANGLES];         // cos(theta)*sin(theta)
  float ang_cmin, ang_cmax;            // min / max of |ang_c| over the evaluated streams
  float mu_c[TUD_MAX_MU];              // -log2(e)*mu
  float mu[TUD_MAX_MU];
  unsigned int mask[TUD_MAX_ALT][TUD_MAX_LAYERS / 32];
  int count[TUD_MAX_ALT];
  const double* gtab;                  // angle-summed transmission function G (tud_g_kernel): [TUDG_NINT][8] doubles
  double g0;                           // G(0) = sum of the quadrature weights
  int skip;                            // tud_g_kernel: an opaque wave may pass over the layers no output sees (TUD_SKIP_* there)
  unsigned char* done;                 // tud_g_kernel<.., .., 1 | 2>: one byte per wave of the shard (the pass in two launches, see there)
  float early_smin;                    // tud_g_kernel<.., .., 1>: a depth below which no downwelling has stopped looking (see there)
};

#define TUD_OPAQUE_Y 26.0f

// ---- building blocks of the TUD kernels -----------------------------------------------------------
// What every lane sets up first. Per-layer constants without a trip to memory inside the layer loop: lane l keeps
// 100 c2 log2(e)/T of layers l and l + 64 and the loop fetches layer k's with two v_readlane (the kernel-argument array
// indexed by the loop counter was a scalar load and its wait -- a few hundred exposed cycles -- in every iteration).
__device__ __forceinline__ double readlane_f64(double v, int lane) {  // lane is wave-uniform
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}
struct TudLane {
  bool live;
  long long i;  // dead lanes shadow the last point: ballots stay wave-wide
  const float* __restrict__ od_col;
  double x, c1x3;
  double ct_a, ct_b;  // set by layer_consts(): a kernel calls it AFTER issuing its first OD loads, so that these loads are
                      // the younger ones and waiting for them (the Planck set-up does at once) leaves no OD load outstanding
  __device__ __forceinline__ explicit TudLane(const TudArgs& a) {
    const long long i_raw = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    live = i_raw < a.g.n;
    i = live ? i_raw : a.g.n - 1;
    od_col = a.OD + i;
    x = grid_x(a.g, a.g.offset + i);
    const double x100 = x * 100.0;
    c1x3 = RT_C1 * (x100 * x100 * x100) * 1e4;
  }
  __device__ __forceinline__ void layer_consts(const TudArgs& a) {
    const int lane_id = threadIdx.x & 63, nL = a.n_layers;
    ct_a = a.c2l2e_over_T[lane_id < nL ? lane_id : 0];
    ct_b = a.c2l2e_over_T[lane_id + 64 < nL ? lane_id + 64 : 0];
  }
  __device__ __forceinline__ double c2l2e_of(int k) const { return readlane_f64(k < 64 ? ct_a : ct_b, k & 63); }  // k wave-uniform
  __device__ __forceinline__ float planck(int k) const { return planck_f32(c1x3, x, c2l2e_of(k)); }
};

// An altitude's layer mask in four scalar registers.
struct LayerMask {
  unsigned w0, w1, w2, w3;
  __device__ __forceinline__ bool bit(int k) const {
    const unsigned w = k < 32 ? w0 : k < 64 ? w1 : k < 96 ? w2 : w3;
    return (w >> (k & 31)) & 1u;
  }
};
__device__ __forceinline__ LayerMask layer_mask(const TudArgs& a, int ia) {
  return LayerMask{a.mask[ia][0], a.mask[ia][1], a.mask[ia][2], a.mask[ia][3]};
}

// One layer of the upwelling recurrence t*Lu + (1-t)*B, y = OD*c: thin lanes through the emissivity, thick lanes through
// the transmittance (the other way round each form cancels: L + e (B - L) with e ~ 1, or t (L - B) + B with t ~ 1).
__device__ __forceinline__ float up_step(float Lu, float B, float y) {
  return (y > -TUD_THIN_Y) ? fmaf(em_thin(y), B - Lu, Lu) : fmaf(__builtin_amdgcn_exp2f(y), Lu - B, B);
}

// How opaque is opaque: what is dropped is at most (transmittance) x (the largest Planck radiance of the column), what
// is kept is at least of the order of the smallest one, so the transmittance has to be 2^-26 of the RATIO of the two
// -- at 6000 cm^-1 between 190 K and 310 K that ratio is 4e7, at 700 cm^-1 it is 8.
__device__ __forceinline__ float opaque_y(const TudArgs& a, const TudLane& l) {
  const float b_hot = planck_f32(l.c1x3, l.x, a.c2l2e_over_Tmax), b_cold = planck_f32(l.c1x3, l.x, a.c2l2e_over_Tmin);
  const float r = __builtin_amdgcn_logf(b_hot / b_cold);  // log2
  return (b_cold > 0.f && r == r && r < 1e30f) ? TUD_OPAQUE_Y + 1.0f + fmaxf(r, 0.f) : 3.0e38f;
}

// Layer loop outside (run-time trip count: any n_layers, no per-n_layers register blow-up), the slant streams
// inside as NA independent recurrences held in registers (full ILP, no dependence between streams). One
// wave-uniform decision per (wave, layer) -- every lane thick / every lane thin / mixed -- picks the cheapest
// exact form for all NA streams of that layer, so the scalar unit sees ~10 instructions per layer, not per stream.
//   opaque: every stream has t <= 2^-26:  L <- B            (1 VALU per stream; most of an opaque band)
//   thick : t = 2^y,             L <- t (L - B) + B          (the fp32 form of :372, 4 VALU per stream)
//   thin  : e = em_thin(y),      L <- L + e (B - L)
//   mixed : per lane, the thin form where |y| < TUD_THIN_Y and the thick form elsewhere
// OD is read once per block of streams, coalesced along the wavenumber axis.
#ifndef TUD_STAGE
#define TUD_STAGE 4  // layers fetched ahead per chunk (tud_g_kernel, C3 column / thinned: 4 -> 0.212 / 0.296 ms, 8 -> 0.219 / 0.305, 16 -> 0.246 / 0.331)
#endif
#ifndef TUD_ABLATE
#define TUD_ABLATE 0  /* timing experiments: 1 = all-thin layers skip the stream updates, 2 = no Planck evaluation, 4 = no up-path */
#endif
#ifndef TUD_ILP
#define TUD_ILP 8  // streams advanced together, step by step, in the all-thick / all-thin layers
#endif
// COL: the whole column of a workgroup's 256 wavenumbers is resident in LDS ([n_layers][256] floats, each thread its own
// slots, so no barrier): every layer's load is issued up front as an LDS-DMA (global_load_lds_dword: no destination
// registers, n_layers loads in flight per wave instead of 8), and the opaque-slab scan, the further (altitude, slant)
// pairs and the main pass all read OD from LDS -- HBM is read exactly once. Up to TUD_COL_LAYERS layers (36 KB per
// workgroup, 4 workgroups per CU); deeper columns (the reference's default 66-layer table) take the chunked form
// (COL = false: TUD_STAGE layers at a time through registers, scan by batched global loads).
#define TUD_COL_LAYERS 36
template <int NA, bool COL>
__global__ __launch_bounds__(256) void tud_kernel(TudArgs a) {
  extern __shared__ float s_od[];  // COL: [n_layers][256]; else [TUD_STAGE][256]
  float (*s_stage)[256] = reinterpret_cast<float (*)[256]>(s_od);
  TudLane ln(a);
  const bool live = ln.live;
  const long long i = ln.i;
  const int nL = a.n_layers;
  const float* __restrict__ od_col = ln.od_col;
  if (COL) {
    float* dst = &s_stage[0][threadIdx.x & ~63u];  // wave-uniform base; the DMA adds lane * 4
    for (int k = 0; k < nL; ++k)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(od_col + (size_t)k * a.ld),
                                       (__attribute__((address_space(3))) void*)(dst + k * 256), 4, 0, 0);
  }
  const double x = ln.x, c1x3 = ln.c1x3;
  if (COL) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the column has landed (this wave's own slots)
  ln.layer_consts(a);
  auto od_at = [&](int k) -> float { return COL ? s_stage[k][threadIdx.x] : od_col[(size_t)k * a.ld]; };
  // COL: at most TUD_COL_LAYERS (< 64) layers, so one register of per-layer constants and no choice between two
  auto planck_of = [&](int k) -> float { return COL ? planck_f32(c1x3, x, readlane_f64(ln.ct_a, k & 63)) : ln.planck(k); };
  const LayerMask mask0 = layer_mask(a, 0);

  // ---- every further (altitude, slant factor) pair: transmittance + upwelling bottom-up (:346-356) ----------
  for (int p = 1; p < a.n_alt * a.n_mu; ++p) {
    const int ia = p / a.n_mu, im = p - ia * a.n_mu;
    const int cnt = a.count[ia];
    const float c = a.mu_c[im];
    float s = 0.f, Lu = 0.f;
    for (int k = 0; k < nL; ++k) {
      const float od = od_at(k);
      if ((a.mask[ia][k >> 5] >> (k & 31)) & 1u) s += od;
      if (k < cnt) {
        Lu = up_step(Lu, planck_of(k), od * c);
      }
    }
    if (live) {
      const size_t o = (size_t)p * (size_t)a.ld_out + (size_t)i;
      a.tau[o] = a.return_od ? s * a.mu[im] : __builtin_amdgcn_exp2f(s * c);
      a.Lu[o] = Lu;
    }
  }
  // ---- downwelling, NA streams at a time, top of the atmosphere downwards (:368-372, 387-388); the first
  //      (altitude, slant) pair rides along with the first block and shares its OD loads and Planck values:
  //      L-up = sum_k (1-t_k) B_k T_k with T_k = 2^(c * sum_{k<j<cnt} OD_j) the transmittance from the top of
  //      layer k to the sensor -- the closed form of the bottom-up recurrence, all terms positive.
  const int nd = a.n_down;
  const int cnt0 = a.count[0];
  const float c0 = a.mu_c[0];
  float s0 = 0.f, S0 = 0.f, Lu0 = 0.f;
  float acc = 0.f;
  const float y_opq = opaque_y(a, ln);
  // Opaque columns. Downwelling at the surface is blind to everything above the lowest slab whose NADIR transmittance
  // is <= 2^-y_opq (what enters it from above reaches the surface attenuated to < 1.5e-8 of the column's own emission, in every stream): find
  // the top of that slab for the whole wave and start the recurrences there. Likewise L-up at the sensor stops
  // collecting once the path above a layer has t <= 2^-26 in every lane. In an absorption band this leaves a few
  // layers at either end of the column; the layers in between only add their OD to the tau sum. In a window
  // (no such slab) the scan costs one extra pass of loads and adds.
  int k_start = nd - 1;
  if (COL) {
    // a lane's prefix sums only grow, so "every lane opaque at layer k" first holds at the largest of the lanes' own first
    // crossings: count, per lane, the prefix sums still below the threshold (no ballots, no branches), then one wave maximum
    float S = 0.f;
    int below = 0;
    for (int k = 0; k < nd; ++k) {
      S += s_stage[k][threadIdx.x];
      below += (S * a.ang_cmin >= y_opq) ? 0 : 1;
    }
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
      const int o = __shfl_xor(below, sh);
      below = o > below ? o : below;
    }
    below = __builtin_amdgcn_readfirstlane(below);  // every lane holds the maximum: tell the compiler it is wave-uniform
    k_start = below < nd - 1 ? below : nd - 1;
  } else {
    float S = 0.f;
    bool found = false;
    // independent loads in flight per step, not one per layer: 2 for the first step (in an absorption band the slab
    // is usually the lowest layer or two), then 8
    for (int k0 = 0, cnt = 2; k0 < nd && !found; k0 += cnt, cnt = 8) {
      float v[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) v[t] = t < cnt ? od_col[(size_t)(k0 + t < nd ? k0 + t : nd - 1) * a.ld] : 0.f;
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        if (!found && t < cnt && k0 + t < nd) {
          S += v[t];
          if (__ballot(S * a.ang_cmin >= y_opq) == ~0ull) {
            k_start = k0 + t;
            found = true;
          }
        }
      }
    }
  }
  bool up_live = true;  // wave-uniform
  for (int a0 = 0; a0 < a.n_ang; a0 += NA) {
    float L[NA], cth[NA];
#pragma unroll
    for (int q = 0; q < NA; ++q) {
      L[q] = 0.f;
      cth[q] = a.ang_c[a0 + q];  // slots past n_ang_real hold the weight-0 nadir stream
    }
    const float c_min = a.ang_cmin, c_max = a.ang_cmax;  // |c| range over the streams (nadir .. most oblique)
    // OD is fetched TUD_STAGE layers at a time: the loads of the next chunk are issued before the current chunk is
    // worked through (8 layers of arithmetic cover the HBM latency; a register rotated one layer ahead does not --
    // the copy that rotates it has to wait for the load) and handed over through the thread's own LDS slots, so the
    // layer loop stays one run-time loop with one copy of the stream code.
    const int k_top = (a0 == 0 ? nL : nd) - 1;
    constexpr int CHUNK = COL ? TUD_MAX_LAYERS : TUD_STAGE;  // COL: one chunk, nothing to restage
    float nxt[TUD_STAGE];
    if (!COL) {
#pragma unroll
      for (int t = 0; t < TUD_STAGE; ++t) nxt[t] = od_col[(size_t)(k_top - t > 0 ? k_top - t : 0) * a.ld];
    }
    for (int kc = k_top; kc >= 0; kc -= CHUNK) {
      if (!COL) {
#pragma unroll
        for (int t = 0; t < TUD_STAGE; ++t) s_stage[t][threadIdx.x] = nxt[t];
#pragma unroll
        for (int t = 0; t < TUD_STAGE; ++t) nxt[t] = od_col[(size_t)(kc - TUD_STAGE - t > 0 ? kc - TUD_STAGE - t : 0) * a.ld];
      }
      const int k_lo = kc - CHUNK + 1 > 0 ? kc - CHUNK + 1 : 0;
    float od_next = COL ? s_stage[kc][threadIdx.x] : s_stage[0][threadIdx.x];
    for (int k = kc; k >= k_lo; --k) {
      const float od = od_next;  // read one layer ahead: the LDS latency hides behind the layer's arithmetic
      if (k > k_lo) od_next = COL ? s_stage[k - 1][threadIdx.x] : s_stage[kc - k + 1][threadIdx.x];
      const bool streams = k <= k_start;                    // wave-uniform (k_start < nd)
      const bool up = !(TUD_ABLATE & 4) && a0 == 0 && up_live && k < cnt0;       // wave-uniform
      if (a0 == 0 && mask0.bit(k)) s0 += od;
      if (!streams && !up) continue;
#if TUD_ABLATE & 2
      const float B = (float)c1x3 * (1e-3f + od);
#else
      const float B = planck_of(k);
#endif
      if (up) {
        Lu0 = fmaf(emissivity(od * c0) * B, __builtin_amdgcn_exp2f(S0 * c0), Lu0);
        S0 += od;
        if (__ballot(S0 * c0 <= -y_opq) == ~0ull) up_live = false;  // c0 < 0
      }
      if (!streams) continue;
      const bool thick = od * c_min >= TUD_THIN_Y;  // even the nadir stream has |y| >= TUD_THIN_Y
      const bool thin = od * c_max < TUD_THIN_Y;    // even the most oblique stream has |y| < TUD_THIN_Y
      // opaque: even the most transparent (nadir) stream has t <= 2^-26: t (L - B) is below half an ulp of B for
      // |L - B| <= 2 B ... and at most 1.5e-8 |L - B| otherwise -- the layer simply replaces L by B
      const bool opaque = od * c_min >= y_opq;
      if (__ballot(opaque) == ~0ull) {
#pragma unroll
        for (int q = 0; q < NA; ++q) L[q] = B;
      } else if (__ballot(thick) == ~0ull) {
        // step-major over blocks of TUD_ILP streams, pinned with scheduling barriers: left to itself the compiler runs the
        // streams' 4-operation chains one after the other (s_nop between dependent packed operations), so a wave never has
        // two independent vector instructions to issue; here every step offers TUD_ILP of them
#pragma unroll
        for (int q0 = 0; q0 < NA; q0 += TUD_ILP) {
          float t[TUD_ILP];
#pragma unroll
          for (int i = 0; i < TUD_ILP; ++i) if (q0 + i < NA) t[i] = od * cth[q0 + i];
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < TUD_ILP; ++i) if (q0 + i < NA) t[i] = __builtin_amdgcn_exp2f(t[i]);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < TUD_ILP; ++i) if (q0 + i < NA) L[q0 + i] = fmaf(t[i], L[q0 + i] - B, B);
          __builtin_amdgcn_sched_barrier(0);
        }
      } else if (__ballot(thin) == ~0ull) {
#if TUD_ABLATE & 1
        L[0] += B * od;
        continue;
#endif
        // 1 - 2^(OD c) as a polynomial in the stream's c with per-lane coefficients A_k = -q_k OD^k (5 multiplies per
        // layer, shared by all streams): 5 VALU per stream instead of forming y and running em_thin (6)
        const float o2 = od * od;
        const float A1 = -EM_Q1 * od, A2 = -EM_Q2 * o2, A3 = -EM_Q3 * (o2 * od), A4 = -EM_Q4 * (o2 * o2);
#pragma unroll
        for (int q0 = 0; q0 < NA; q0 += TUD_ILP) {  // step-major, as above
          float e[TUD_ILP];
#pragma unroll
          for (int i = 0; i < TUD_ILP; ++i) if (q0 + i < NA) e[i] = fmaf(cth[q0 + i], A4, A3);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < TUD_ILP; ++i) if (q0 + i < NA) e[i] = fmaf(cth[q0 + i], e[i], A2);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < TUD_ILP; ++i) if (q0 + i < NA) e[i] = fmaf(cth[q0 + i], e[i], A1);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < TUD_ILP; ++i) if (q0 + i < NA) e[i] = cth[q0 + i] * e[i];
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < TUD_ILP; ++i) if (q0 + i < NA) L[q0 + i] = fmaf(e[i], B - L[q0 + i], L[q0 + i]);
          __builtin_amdgcn_sched_barrier(0);
        }
      } else {
        // Mixed layer: neither form holds for every lane AND every stream. The slant factors span 1 .. 19, so a layer
        // with OD between 0.005 and 0.09 lands here even when all 64 lanes agree; only where the lanes themselves
        // straddle the switch does a lane need both forms. So the form is chosen per block of 4 consecutive streams
        // (|c| ascends with the stream index): all lanes thick for the block's most transparent stream -> transmittance
        // form; all lanes thin for its most oblique one -> emissivity polynomial; else both forms and a per-lane select.
        const float o2 = od * od;
        const float A1 = -EM_Q1 * od, A2 = -EM_Q2 * o2, A3 = -EM_Q3 * (o2 * od), A4 = -EM_Q4 * (o2 * o2);
#pragma unroll
        for (int q0 = 0; q0 < NA; q0 += 4) {
          // |c| ascends with the stream index (pads repeat the last stream): the block's extremes are its end streams,
          // already in scalar registers -- fetching per-block bounds from the kernel arguments here put a scalar load
          // and its wait in front of every block
          const int q1 = q0 + 3 < NA ? q0 + 3 : NA - 1;
          const bool blk_thick = __ballot(od * -cth[q0] >= TUD_THIN_Y) == ~0ull;
          const bool blk_thin = __ballot(od * -cth[q1] < TUD_THIN_Y) == ~0ull;
          const int nq = q0 + 4 < NA ? 4 : NA - q0;  // streams of this block (compile-time after unrolling)
          float w[4];
          // the block's 4 streams advance together, step by step (scheduling barriers pin the order: four independent
          // instructions per step instead of four serial chains)
          if (blk_thick) {
#pragma unroll
            for (int i = 0; i < 4; ++i) if (i < nq) w[i] = od * cth[q0 + i];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 4; ++i) if (i < nq) w[i] = __builtin_amdgcn_exp2f(w[i]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 4; ++i) if (i < nq) L[q0 + i] = fmaf(w[i], L[q0 + i] - B, B);
          } else if (blk_thin) {
#pragma unroll
            for (int i = 0; i < 4; ++i) if (i < nq) w[i] = fmaf(cth[q0 + i], A4, A3);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 4; ++i) if (i < nq) w[i] = fmaf(cth[q0 + i], w[i], A2);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 4; ++i) if (i < nq) w[i] = fmaf(cth[q0 + i], w[i], A1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 4; ++i) if (i < nq) w[i] = cth[q0 + i] * w[i];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 4; ++i) if (i < nq) L[q0 + i] = fmaf(w[i], B - L[q0 + i], L[q0 + i]);
          } else {
            // per lane: thin through the emissivity, L + e (B - L); thick through the transmittance, B - t (B - L) (each form
            // cancels in the other regime). Branch-free: one shared B - L, selects on the factor and on the base -- the same
            // bits as the two fmaf forms (fl(B - L) = -fl(L - B)).
            float y[4], t[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) if (i < nq) y[i] = od * cth[q0 + i];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 4; ++i) if (i < nq) { t[i] = __builtin_amdgcn_exp2f(y[i]); w[i] = em_thin(y[i]); }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 4; ++i) if (i < nq) {
              const bool thin_lane = y[i] > -TUD_THIN_Y;
              L[q0 + i] = fmaf(thin_lane ? w[i] : -t[i], B - L[q0 + i], thin_lane ? L[q0 + i] : B);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    }
#pragma unroll
    for (int q = 0; q < NA; ++q) {
      acc = fmaf(L[q], a.ang_w[a0 + q], acc);
      if (a.Ld_ang && live && a0 + q < a.n_ang_real) a.Ld_ang[(size_t)(a0 + q) * a.ld_out + i] = L[q];
    }
  }
  if (live) {
    a.tau[i] = a.return_od ? s0 * a.mu[0] : __builtin_amdgcn_exp2f(s0 * c0);
    a.Lu[i] = Lu0;
    a.Ld[i] = acc * a.inv_wsum;
  }
}

// ---------------------------------------------------------------------------------------------------
// Downwelling without streams. Unrolled, stream q's recurrence (:368-372) is
//   L_q = sum_k B_k (1 - t_kq) prod_{j<k} t_jq = sum_k B_k [ exp(-S_k sec_q) - exp(-S_{k+1} sec_q) ],
// S_k = the optical depth between the surface and the bottom of layer k, so the weighted sum over the streams (:387-388) is
//   sum_q w_q L_q = sum_k B_k [ G(S_k) - G(S_{k+1}) ],     G(S) = sum_q w_q exp(-S / cos(theta_q)),
// the reference's own quadrature regrouped: ONE function of one variable, fixed by N_angle, evaluated at n_layers + 1
// depths per wavenumber instead of (N_angle - 1) x n_layers stream updates. G is a sum of 29 decaying exponentials with rates
// 1 .. 19; the host tabulates it once per N_angle as piecewise degree-6 polynomials (fp64 Chebyshev interpolants, 225
// intervals: 16 per binade of S + 2^-6 below S = 16, width 1/2 above, nothing beyond 48 where G < 1e-20 G(0)) to 4e-14 of
// G(0), and the kernel evaluates it in fp64, so the differences G(S_k) - G(S_{k+1}) keep their relative accuracy down to
// layers of OD ~ 1e-9 with no thin / thick / mixed case distinction at all (the stream kernel needed three forms of
// 1 - t for that). Cost per wavenumber and layer: one fp64 Horner of degree 6 + an index + 4 LDS reads instead of 29 x 6
// fp32 operations. The per-stream radiances themselves (opts['save']) still come from the stream kernel.
#define TUDG_M 4                     // 2^M intervals per binade of (S + TUDG_OFF) below TUDG_SWITCH
#define TUDG_OFF 0.015625f           // 2^-6
#define TUDG_SWITCH 16.0f
#define TUDG_SMAX 48.0
#define TUDG_DEG 6
#define TUDG_BASE (0x3C800000 >> (23 - TUDG_M))   // bits of 2^-6, shifted
#define TUDG_NLOG ((0x41800000 >> (23 - TUDG_M)) - TUDG_BASE + 1)  // log-spaced intervals: bits of 16 -> the last one
#define TUDG_NINT (TUDG_NLOG + (int)((TUDG_SMAX - 16.0) * 2.0))

__device__ __forceinline__ int tudg_index(float sf) {
  const int il = (__float_as_int(sf + TUDG_OFF) >> (23 - TUDG_M)) - TUDG_BASE;
  const int iu = TUDG_NLOG + (int)((sf - TUDG_SWITCH) * 2.0f);
  int idx = sf < TUDG_SWITCH ? il : iu;
  idx = idx < 0 ? 0 : idx;
  return idx < TUDG_NINT - 1 ? idx : TUDG_NINT - 1;
}
__device__ __forceinline__ double tudg_eval(const double* __restrict__ s_g, double S) {
  const double Sc = fmin(S, TUDG_SMAX);  // (a NaN depth is flagged by the caller)
  const int idx = tudg_index((float)Sc);
  const double2* __restrict__ p = reinterpret_cast<const double2*>(s_g + idx * 8);
  const double2 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];  // mid a0 | a1 a2 | a3 a4 | a5 a6
  const double u = Sc - q0.x;
  double r = q3.y;
  r = fma(r, u, q3.x); r = fma(r, u, q2.y); r = fma(r, u, q2.x);
  r = fma(r, u, q1.y); r = fma(r, u, q1.x); r = fma(r, u, q0.y);
  return r;
}

// Planck radiances of a layer across the 64 consecutive wavenumbers of a wave: B(nu, T_k) is so smooth in nu that a parabola
// through its values at lanes 0, 32 and 63 reproduces it to < 1e-10 on grids this fine (the host checks
// (4/nu_min + c2/T_min) x 63 steps <= 7e-3 and launches the PN = false instantiations otherwise). The three values of EVERY layer are
// computed in one go with lane = layer (lane k already holds layer k's 100 c2 log2e / T): 3 Planck evaluations per wave
// instead of one per layer, and the layer loop rebuilds B_k with two FMAs on coefficients fetched by v_readlane.
struct PlanckNodes {
  float c0, c1, c2;     // lane k: coefficients of layer k in t = lane / 63
  float c0b, c1b, c2b;  // ... of layer k + 64
  float t;
};
__device__ __forceinline__ PlanckNodes planck_nodes_setup(const TudArgs& a, const TudLane& l) {
  PlanckNodes P;
  const double ct_a = l.ct_a, ct_b = l.ct_b;
  const int nL = a.n_layers;
  const long long i0w = (long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63u);  // raw index of lane 0 (may lie past the shard: grid_x extrapolates)
  const float t1 = 32.0f / 63.0f;
  float b[3], bb[3];
#pragma unroll
  for (int n = 0; n < 3; ++n) {
    const double xn = grid_x(a.g, a.g.offset + i0w + (n == 0 ? 0 : n == 1 ? 32 : 63));
    const double x100 = xn * 100.0;
    const double c1x3 = RT_C1 * (x100 * x100 * x100) * 1e4;
    b[n] = planck_f32(c1x3, xn, ct_a);
    bb[n] = nL > 64 ? planck_f32(c1x3, xn, ct_b) : 0.f;  // wave-uniform branch
  }
  // Newton form through (0, b0), (t1, b1), (1, b2), expanded to monomials
  {
    const float d01 = (b[1] - b[0]) / t1, d12 = (b[2] - b[1]) / (1.0f - t1);
    P.c2 = d12 - d01; P.c1 = d01 - P.c2 * t1; P.c0 = b[0];
  }
  {
    const float d01 = (bb[1] - bb[0]) / t1, d12 = (bb[2] - bb[1]) / (1.0f - t1);
    P.c2b = d12 - d01; P.c1b = d01 - P.c2b * t1; P.c0b = bb[0];
  }
  P.t = (float)(threadIdx.x & 63) * (1.0f / 63.0f);
  return P;
}
// B of the layer whose coefficients sit in lane `lane` of the first (hi = false) or second register set; both wave-uniform.
// The unrolled chunks pass a static lane offset and one choice of set per chunk.
__device__ __forceinline__ float planck_nodes_eval(const PlanckNodes& P, bool hi, int lane) {
  const float c0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(hi ? P.c0b : P.c0), lane));
  const float c1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(hi ? P.c1b : P.c1), lane));
  const float c2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(hi ? P.c2b : P.c2), lane));
  return fmaf(fmaf(c2, P.t, c1), P.t, c0);
}
__device__ __forceinline__ float planck_nodes_eval(const PlanckNodes& P, int k) {  // k wave-uniform: a branch, not three selects
  if (k < 64) return planck_nodes_eval(P, false, k);
  return planck_nodes_eval(P, true, k - 64);
}

__device__ __forceinline__ void tudg_load(double* s_g, const TudArgs& a) {  // the G table into LDS; __syncthreads() before use
  for (int t = threadIdx.x; t < TUDG_NINT * 4; t += 256) reinterpret_cast<double2*>(s_g)[t] = reinterpret_cast<const double2*>(a.gtab)[t];
}

// The downwelling sum_k B_k [G(S_k) - G(S_k+1)], bottom-up. Downwelling at the surface is blind to everything above the
// depth where G has dropped to 2^-27 of G(0) times the column's Planck dynamic range at this wavenumber (what is dropped is
// at most that transmission times the largest Planck radiance, what is kept is of the order of the smallest): once every
// lane is there the wave stops evaluating G.
struct TudDown {
  double S, g_prev, g_floor;
  float acc;
  bool live;  // wave-uniform
  __device__ __forceinline__ TudDown(const double* s_g, const TudArgs& a, const TudLane& l) {
    S = 0.0;
    g_prev = tudg_eval(s_g, 0.0);  // (not a.g0: the table's own value, so that an empty column gives exactly 0)
    acc = 0.f;
    g_floor = a.g0 * (double)__builtin_amdgcn_exp2f(-fminf(opaque_y(a, l), 120.0f));
    live = a.n_down > 0;
  }
  __device__ __forceinline__ TudDown(const double* s_g, const TudArgs& a, float y_opq) {  // y_opq = opaque_y(a, lane)
    S = 0.0;
    g_prev = tudg_eval(s_g, 0.0);
    acc = 0.f;
    g_floor = a.g0 * (double)__builtin_amdgcn_exp2f(-fminf(y_opq, 120.0f));
    live = a.n_down > 0;
  }
  __device__ __forceinline__ void step(const double* s_g, float od, float B) {
    S += (double)od;
    const double g = tudg_eval(s_g, S);
    acc = fmaf(B, (float)(g_prev - g), acc);
    g_prev = g;
    if (__ballot(g > g_floor) == 0ull) live = false;
  }
  __device__ __forceinline__ float result(const TudArgs& a) const {  // a NaN optical depth poisons the sum, as in the reference
    return (S != S) ? __builtin_nanf("") : acc * a.inv_wsum;
  }
};

// The layers an opaque column hides from every output (tud_g_kernel, at the end of its chunk loop)
// layers below the sensor a wave looks at: the top chunk in registers and two chunks in the 2 * TUD_STAGE LDS slots of a
// thread -- not a knob, the look is laid out for exactly this (tools/count_tud_layers.py for what other limits would give)
#define TUD_SKIP_SCAN (3 * TUD_STAGE)
// a wave looks only if its downwelling has died (or run out of layers) within this many layers: on the C3 column every wave
// that finds its top opaque is such a wave, and of the waves of the thinned columns that would look in vain (mixing ratios
// x 1e-1: 73 %) most die later (tools/count_tud_layers.py)
#define TUD_SKIP_BOTTOM TUD_STAGE
#define TUD_SKIP_MARGIN 8.0f  // beyond opaque_y: what L-up drops is <= 2^-11 ulp of what it keeps
#define TUD_SKIP_TAU0 151.0f  // exp2f(-y) is exactly 0 from y = 150 on; one more for fp32 sums taken in another order

// SKIP: the instantiation that may look (launched only with a.skip, and only with PN). Without it every line below that
// serves the look is compiled out and the kernel is the one it was before the look existed, instruction for instruction.
//
// PHASE: the same pass in two launches around the line-sum of the middle layers (rtx_compute_tud_opts, RTX_CTUD_OD_SCRATCH).
// A wave decides from layers [0, TUD_SKIP_BOTTOM) and [k_top - (TUD_SKIP_SCAN - TUD_STAGE), cnt0) alone whether it skips, and
// where the tau loop stops before its first load it reads no other layer at all. PHASE 1 (early) runs when only those layers
// have been summed: such a wave finishes as it always does, stores its outputs and writes done[wave] = 1; every other wave
// (a downwelling alive after the first chunk, a look that finds nothing, a look that has to sum middle chunks) writes
// done[wave] = 0 and returns without storing. The line-sum of the middle layers then leaves out the rows of the done waves,
// and PHASE 2 (late) runs the whole pass for the waves that are not done. Either way a wave executes the instruction sequence
// of PHASE 0 on the same data, in one launch or the other: tau, L-up and L-down keep their bits. PHASE 0 is the kernel every
// other call launches; the lines that serve the phases are compiled out of it.
template <bool PN, bool SKIP, int PHASE = 0>
__global__ __launch_bounds__(256) void tud_g_kernel(TudArgs a) {
  static_assert(PN || !SKIP, "the look at the top is written for the Planck-node instantiation");
  static_assert(PHASE == 0 || SKIP, "the two-launch pass belongs to the instantiation that may look");
  __shared__ double s_g[TUDG_NINT * 8];
  __shared__ float s_stage[(SKIP ? 2 : 1) * TUD_STAGE][256];  // each thread's own slots: the first TUD_STAGE hand the chunks over, all of them serve the look at the top
  // late: the workgroup's four flags in one scalar load (the array is padded to whole workgroups and early wrote every entry)
  unsigned done4 = 0u;
  if (PHASE == 2) {
    done4 = reinterpret_cast<const unsigned*>(a.done)[blockIdx.x];
    if (done4 == 0x01010101u) return;
  }
  // early, on a column that hides nothing: the launch must cost next to nothing there, and a wave's set-up (the G table, eight
  // fp64 Planck values) and its first chunk are most of what a full pass of a thin column costs per layer. A wave can be done
  // only if its downwelling has stopped looking after the first chunk, G(S) <= G(0) 2^-opaque_y with opaque_y >= 27 in every
  // lane, hence only if the depth of that chunk is at least early_smin (the host solves G(S) = G(0) 2^-26.5 and takes a
  // little off for the fp32 sum; -inf where the downwelling can run out of layers instead). The workgroup whose four waves
  // all fail that says so and returns before the table is loaded; any other runs on as it is, and its waves decide as always.
  if (PHASE == 1) {
    __shared__ int s_may[4];
    const long long i_pre = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const float* __restrict__ od_pre = a.OD + (i_pre < a.g.n ? i_pre : a.g.n - 1);
    float s_pre = 0.f;
#pragma unroll
    for (int t = 0; t < TUD_STAGE; ++t) s_pre += od_pre[(size_t)(t < a.n_layers ? t : a.n_layers - 1) * a.ld];
    const bool may = __ballot(s_pre >= a.early_smin) == ~0ull;
    if ((threadIdx.x & 63) == 0) s_may[threadIdx.x >> 6] = may ? 1 : 0;
    __syncthreads();
    if (!(s_may[0] | s_may[1] | s_may[2] | s_may[3])) {
      if ((threadIdx.x & 63) == 0) a.done[(size_t)blockIdx.x * 4 + (threadIdx.x >> 6)] = 0;
      return;
    }
  }
  tudg_load(s_g, a);
  TudLane ln(a);
  const int nL = a.n_layers;
  const float* __restrict__ od_col = ln.od_col;
  // The staged OD fetch (these loads, the bumped pointers and the hand-over at the top of the chunk loop) is spelled out here
  // and in tud_g_snap_kernel, not shared: as a struct or as functions taking the arrays it compiled to another chunk loop
  // (other branch structure and waits, generic loads in one form), and this loop is the one bound by the scalar unit.
  float nxt[TUD_STAGE];
#pragma unroll
  for (int t = 0; t < TUD_STAGE; ++t) nxt[t] = od_col[(size_t)(t < nL ? t : nL - 1) * a.ld];
  ln.layer_consts(a);
  const LayerMask mask0 = layer_mask(a, 0);
  PlanckNodes PNd;
  if (PN) PNd = planck_nodes_setup(a, ln);
  __syncthreads();  // the table is in LDS
  // (a done wave of a workgroup that still has work leaves here: the table load above is the whole workgroup's)
  if (PHASE == 2 && ((done4 >> (8 * (threadIdx.x >> 6))) & 1u)) return;
  auto not_done = [&]() {
    if ((threadIdx.x & 63) == 0) a.done[(size_t)blockIdx.x * 4 + (threadIdx.x >> 6)] = 0;
  };

  // ---- every further (altitude, slant factor) pair: transmittance + upwelling bottom-up (:346-356) ----------
  for (int p = 1; p < a.n_alt * a.n_mu; ++p) {
    const int ia = p / a.n_mu, im = p - ia * a.n_mu;
    const int cnt = a.count[ia];
    const float c = a.mu_c[im];
    float s = 0.f, Lu = 0.f;
    for (int k = 0; k < nL; ++k) {
      const float od = ln.od_col[(size_t)k * a.ld];
      if ((a.mask[ia][k >> 5] >> (k & 31)) & 1u) s += od;
      if (k < cnt) Lu = up_step(Lu, PN ? planck_nodes_eval(PNd, k) : ln.planck(k), od * c);
    }
    if (ln.live) {
      const size_t o = (size_t)p * (size_t)a.ld_out + (size_t)ln.i;
      a.tau[o] = a.return_od ? s * a.mu[im] : __builtin_amdgcn_exp2f(s * c);
      a.Lu[o] = Lu;
    }
  }

  // ---- the first pair's transmittance and upwelling, and the downwelling, in one bottom-up pass -------------------------
  const int nd = a.n_down, cnt0 = a.count[0];
  const float c0 = a.mu_c[0];
  float s0 = 0.f, Lu0 = 0.f;
  // (SKIP: opaque_y once -- its two Planck values are fp64 work, and the look at the top wants it too)
  const float y_opq = SKIP ? opaque_y(a, ln) : 0.f;
  TudDown down = SKIP ? TudDown(s_g, a, y_opq) : TudDown(s_g, a, ln);
  bool skip_armed = SKIP;  // wave-uniform: the hidden layers (below the chunk loop) have not been looked for yet
  // The layer loop is bound by the CU's one scalar unit, not by HBM or the vector ALUs (round 3: 1.04e8 scalar against
  // 1.19e8 vector instructions per launch, ~45 scalar instructions per layer: 64-bit index products for the prefetch
  // addresses, the 128-bit mask lookup, the up / down flags, the loop control of a run-time inner loop). So: the prefetch
  // pointers are bumped instead of recomputed, and a chunk of TUD_STAGE layers that all count for the upwelling
  // and the downwelling (every chunk of the C3 column) runs unrolled with static layer offsets and a chunk-level mask word.
  const unsigned long long m_lo = (unsigned long long)mask0.w0 | ((unsigned long long)mask0.w1 << 32);
  const unsigned long long m_hi = (unsigned long long)mask0.w2 | ((unsigned long long)mask0.w3 << 32);
  const size_t bump = (size_t)TUD_STAGE * (size_t)a.ld;
  const float y_up = y_opq + TUD_SKIP_MARGIN;
  const int k_top = (cnt0 - 1) & ~(TUD_STAGE - 1);  // the chunk that holds layer cnt0 - 1
  int k_look = -1;  // >= 0: the chunk loop was left before layer k_look for the look at the top of the column, below it
  const float* pf[TUD_STAGE];
#pragma unroll
  for (int t = 0; t < TUD_STAGE; ++t) pf[t] = od_col + (size_t)(TUD_STAGE + t) * (size_t)a.ld;
  for (int kc = 0; kc < nL; kc += TUD_STAGE) {
#pragma unroll
    for (int t = 0; t < TUD_STAGE; ++t) s_stage[t][threadIdx.x] = nxt[t];
    if (kc + 2 * TUD_STAGE <= nL) {
#pragma unroll
      for (int t = 0; t < TUD_STAGE; ++t) nxt[t] = *pf[t];
    } else {
#pragma unroll
      for (int t = 0; t < TUD_STAGE; ++t)
        if (kc + TUD_STAGE + t < nL) nxt[t] = *pf[t];
    }
#pragma unroll
    for (int t = 0; t < TUD_STAGE; ++t) pf[t] += bump;
    const int k_hi = kc + TUD_STAGE < nL ? kc + TUD_STAGE : nL;
    if (PN && k_hi == kc + TUD_STAGE && k_hi <= cnt0 && k_hi <= nd) {
      const unsigned mchunk = (unsigned)((kc < 64 ? m_lo : m_hi) >> (kc & 63));  // kc is a multiple of TUD_STAGE: no straddle
      const bool hi_set = kc >= 64;
#pragma unroll
      for (int t = 0; t < TUD_STAGE; ++t) {
        const float od = s_stage[t][threadIdx.x];
        if ((mchunk >> t) & 1u) s0 += od;
        const float B = planck_nodes_eval(PNd, hi_set, (kc & 63) + t);
        Lu0 = up_step(Lu0, B, od * c0);
        if (down.live) down.step(s_g, od, B);
      }
      // (this loop is bound by the scalar unit: where the downwelling lives on, one flag is tested per chunk and no more.
      //  A downwelling that runs out of layers exactly at the end of the first chunk, n_down == TUD_STAGE < count, alive, is
      //  therefore not seen here, and the other branch sees it a chunk too late for TUD_SKIP_BOTTOM: such a wave never looks)
      if (SKIP && !down.live) {
        if (skip_armed) {
          skip_armed = false;
          if (k_hi <= TUD_SKIP_BOTTOM && k_hi + TUD_STAGE <= k_top) { k_look = k_hi; break; }
        }
      }
    } else {
      for (int k = kc; k < k_hi; ++k) {
        const float od = s_stage[k - kc][threadIdx.x];
        if (mask0.bit(k)) s0 += od;
        const bool up = k < cnt0, dn = down.live && k < nd;  // wave-uniform
        if (!up && !dn) continue;
        const float B = PN ? planck_nodes_eval(PNd, k) : ln.planck(k);
        if (up) Lu0 = up_step(Lu0, B, od * c0);
        if (dn) down.step(s_g, od, B);
      }
      // the downwelling has stopped looking, or has run out of layers, within the first TUD_SKIP_BOTTOM layers, with a chunk to
      // save below a chunk to look at (a wave is asked once: later chunks see skip_armed false)
      if (SKIP && skip_armed && !(down.live && k_hi < nd)) {
        skip_armed = false;
        if (k_hi <= TUD_SKIP_BOTTOM && k_hi + TUD_STAGE <= k_top) { k_look = k_hi; break; }
      }
    }
    if (PHASE == 1) break;  // early: a wave that has not left for the look by now needs layers that are not there yet
  }
  if (PHASE == 1 && k_look < 0) { not_done(); return; }
  // ---- the layers an opaque column hides from every output -----------------------------------------------------------
  // a.skip: the caller vouches that every OD is finite and >= 0, tau (not the depth) is asked for, and the mask is the
  // first cnt0 layers. The wave looks at the top TUD_SKIP_SCAN layers of the column, fetched in one go (the loop above is
  // bound by its chain of dependent fetches, TUD_STAGE loads per lane in flight: a look that took its chunks one round
  // trip after the other cost what it saved), for the highest chunk boundary k_res above which EVERY lane has an optical
  // path of opaque_y + TUD_SKIP_MARGIN to the sensor. L-up at the sensor holds nothing of what lies below it: what enters
  // layer k_res from below lies within the column's Planck range and arrives attenuated by 2^-(26 + 1 + 8) B_cold /
  // B_hot, i.e. <= 2^-35 B_cold, 2^-11 ulp of anything the top can emit. The chunks in between count for the tau sum
  // alone -- no Planck value, no up_step -- and not even for that once bottom + top put the sum past TUD_SKIP_TAU0 in
  // every lane: the layers left out, being >= 0, only add to it. The pass then finishes from k_res out of the registers
  // and LDS slots the look filled. So s0 is the complete bottom-up sum in its order, or maps to 0 as the complete sum does: tau and
  // L-down keep their bits, L-up moves by <= 2^-35 B_cold before rounding. Decided once per wave and on whole chunks, and
  // only by a wave whose downwelling is done within TUD_SKIP_BOTTOM layers (the others rarely find an opaque top). A
  // wave whose downwelling lives to the top -- every window, every thin column -- tests one flag per chunk and never
  // comes here; one that finds nothing runs the rest of the column as before, its next chunk having been in flight all
  // along -- in a copy of the loop without the downwelling, which is done either way (coming back into the loop above
  // kept that loop's whole state alive across the look: ten registers, a wave per SIMD). A NaN in a layer looked at
  // fails the comparison: no skip.
  if (SKIP && k_look >= 0) {
    int kc = k_look;  // the first layer not yet run
    // (the column's address is formed again from the thread's index: TudLane's would hold two registers through the loop above)
    unsigned tid_top = threadIdx.x;
    asm volatile("" : "+v"(tid_top));  // (kept apart from TudLane's index, or the two are merged again)
    const long long i_top = (long long)blockIdx.x * blockDim.x + tid_top;
    const float* __restrict__ od_top = a.OD + (i_top < a.g.n ? i_top : a.g.n - 1);
    constexpr int NC = TUD_SKIP_SCAN / TUD_STAGE;
    const float ac0 = -c0;
    const int k_deep = k_top - (TUD_SKIP_SCAN - TUD_STAGE);
    const int k_scan = k_deep > kc + TUD_STAGE ? k_deep : kc + TUD_STAGE;  // kc: the first layer not yet run
    // the top chunk into registers (it may be ragged), the two below it straight into the thread's own LDS slots (LDS-DMA:
    // no destination registers -- twelve more live values would cost the kernel a wave per SIMD): chunk 1 into the upper
    // slots, chunk 2 into the hand-over slots, which are free between two chunks of the loop
    static_assert(NC == 3, "the look at the top is laid out for three chunks");
    float v0[TUD_STAGE];
#pragma unroll
    for (int t = 0; t < TUD_STAGE; ++t) v0[t] = od_top[(size_t)(k_top + t < cnt0 ? k_top + t : cnt0 - 1) * (size_t)a.ld];
    {
      // (a rolled loop over one walking pointer: unrolled, the eight addresses were all formed first and took sixteen registers)
      float* dst = &s_stage[0][threadIdx.x & ~63u];  // wave-uniform base; the DMA adds lane * 4
      const int n_dma = k_top - 2 * TUD_STAGE >= k_scan ? 2 * TUD_STAGE : k_top - TUD_STAGE >= k_scan ? TUD_STAGE : 0;
      const float* pc = od_top + (size_t)(k_top - n_dma) * (size_t)a.ld;  // layer k_top - n_dma + j -> slot j (+ TUD_STAGE with one chunk)
      float* d = dst + (n_dma == TUD_STAGE ? TUD_STAGE * 256 : 0);
#pragma unroll 1
      for (int j = 0; j < n_dma; ++j) {
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)pc, (__attribute__((address_space(3))) void*)d, 4, 0, 0);
        pc += a.ld;
        d += 256;
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the DMA has landed (this wave's own slots)
    float s_top = 0.f;
#pragma unroll
    for (int t = TUD_STAGE - 1; t >= 0; --t)
      if (k_top + t < cnt0) s_top += v0[t];
    int k_res = -1;  // the chunk the pass goes on from
    if (__ballot(s_top * ac0 >= y_up) == ~0ull) k_res = k_top;
#pragma unroll 1
    for (int c = 1; c < NC && k_res < 0 && k_top - c * TUD_STAGE >= k_scan; ++c) {
      const int slot = c == 1 ? TUD_STAGE : 0;
#pragma unroll
      for (int t = TUD_STAGE - 1; t >= 0; --t) s_top += s_stage[slot + t][threadIdx.x];
      if (__ballot(s_top * ac0 >= y_up) == ~0ull) k_res = k_top - c * TUD_STAGE;
    }
    if (PHASE == 1) {  // early: done only where the tau loop below stops before its first load
      if (k_res < 0 || (kc < k_res && __ballot((s0 + s_top) * ac0 >= TUD_SKIP_TAU0) != ~0ull)) { not_done(); return; }
      if ((threadIdx.x & 63) == 0) a.done[(size_t)blockIdx.x * 4 + (threadIdx.x >> 6)] = 1;
    }
    if (k_res < 0) {  // nothing found: on with the column at kc, whose chunk has been in flight into nxt all along
#pragma unroll
      for (int t = 0; t < TUD_STAGE; ++t) pf[t] = od_top + (size_t)(kc + TUD_STAGE + t) * (size_t)a.ld;
      for (; kc < cnt0; kc += TUD_STAGE) {
#pragma unroll
        for (int t = 0; t < TUD_STAGE; ++t) s_stage[t][threadIdx.x] = nxt[t];
#pragma unroll
        for (int t = 0; t < TUD_STAGE; ++t)
          if (kc + TUD_STAGE + t < cnt0) nxt[t] = *pf[t];
#pragma unroll
        for (int t = 0; t < TUD_STAGE; ++t) pf[t] += bump;
        if (kc + TUD_STAGE <= cnt0) {  // (prefix mask: every layer below cnt0 counts for tau)
          const bool hi_set = kc >= 64;
#pragma unroll
          for (int t = 0; t < TUD_STAGE; ++t) {
            const float od = s_stage[t][threadIdx.x];
            s0 += od;
            Lu0 = up_step(Lu0, planck_nodes_eval(PNd, hi_set, (kc & 63) + t), od * c0);
          }
        } else {
          for (int k = kc; k < cnt0; ++k) {
            const float od = s_stage[k - kc][threadIdx.x];
            s0 += od;
            Lu0 = up_step(Lu0, planck_nodes_eval(PNd, k), od * c0);
          }
        }
      }
    } else {
    for (int km = kc; km < k_res; km += TUD_STAGE) {  // kc and k_res are chunk boundaries, every layer here < cnt0
      if (__ballot((s0 + s_top) * ac0 >= TUD_SKIP_TAU0) == ~0ull) break;
      float w[TUD_STAGE];
#pragma unroll
      for (int t = 0; t < TUD_STAGE; ++t) w[t] = od_top[(size_t)(km + t) * (size_t)a.ld];
#pragma unroll
      for (int t = 0; t < TUD_STAGE; ++t) s0 += w[t];
    }
#pragma unroll 1
    for (int kb = k_res; kb < k_top; kb += TUD_STAGE) {  // whole chunks out of the LDS slots
      const int slot = kb == k_top - TUD_STAGE ? TUD_STAGE : 0;
#pragma unroll
      for (int t = 0; t < TUD_STAGE; ++t) {
        const float od = s_stage[slot + t][threadIdx.x];
        s0 += od;
        Lu0 = up_step(Lu0, planck_nodes_eval(PNd, kb + t), od * c0);
      }
    }
#pragma unroll
    for (int t = 0; t < TUD_STAGE; ++t) {  // the top chunk out of its registers
      if (k_top + t < cnt0) {
        s0 += v0[t];
        Lu0 = up_step(Lu0, planck_nodes_eval(PNd, k_top + t), v0[t] * c0);
      }
    }
    }  // (layers from cnt0 on count for nothing here: prefix mask, and the downwelling is done)
  }
  // (SKIP: the point's index is formed again here, kept apart from TudLane's: that copy would hold two registers through both loops)
  long long i_out = ln.i;
  bool live_out = ln.live;
  if (SKIP) {
    unsigned tid_out = threadIdx.x;
    asm volatile("" : "+v"(tid_out));
    i_out = (long long)blockIdx.x * blockDim.x + tid_out;
    live_out = i_out < a.g.n;
  }
  if (live_out) {
    a.tau[i_out] = a.return_od ? s0 * a.mu[0] : __builtin_amdgcn_exp2f(s0 * c0);
    a.Lu[i_out] = Lu0;
    a.Ld[i_out] = down.result(a);
  }
}

// PB = (altitude, slant) pairs advanced together in one bottom-up pass: they share the OD loads and the Planck values (the
// reference's main caller asks for 9 sensor altitudes, Generate_LWIR_TUD.py:81; one pass per pair recomputed B for each).
// A single pair takes tud_g_kernel above; several run here in blocks of PB = TUDG_PB (84 registers), the first block
// carrying the downwelling.
#ifndef TUDG_PB
#define TUDG_PB 3  // 9 pairs, ms: blocks of 2 -> 1.29, 3 -> 1.01, 4 -> 1.15, 8 -> 1.32 (one pass per pair: 1.41)
#endif
template <int PB>
__global__ __launch_bounds__(256) void tud_g_pairs_kernel(TudArgs a) {
  __shared__ double s_g[TUDG_NINT * 8];
  __shared__ float s_stage[TUD_STAGE][256];  // each thread's own slots
  tudg_load(s_g, a);
  TudLane ln(a);
  const int nL = a.n_layers;
  const float* __restrict__ od_col = ln.od_col;
  ln.layer_consts(a);
  __syncthreads();  // the table is in LDS

  const int nd = a.n_down;
  const int npair = a.n_alt * a.n_mu;
  TudDown down(s_g, a, ln);

  // ---- transmittance and upwelling of PB (altitude, slant) pairs bottom-up (:346-356); the first block also carries the
  //      downwelling --------------------------------------------------------------------------------------------------------
  for (int p0 = 0; p0 < npair; p0 += PB) {
    float cp[PB], mup[PB];
    int cntp[PB];
    unsigned mw[PB][TUD_MAX_LAYERS / 32];
    int cnt_max = 0;
#pragma unroll
    for (int j = 0; j < PB; ++j) {  // wave-uniform constants of the block's pairs
      const int p = p0 + j < npair ? p0 + j : p0;
      const int ia = p / a.n_mu, im = p - ia * a.n_mu;
      cp[j] = a.mu_c[im];
      mup[j] = a.mu[im];
      cntp[j] = p0 + j < npair ? a.count[ia] : 0;
#pragma unroll
      for (int w = 0; w < TUD_MAX_LAYERS / 32; ++w) mw[j][w] = p0 + j < npair ? a.mask[ia][w] : 0u;
      cnt_max = cntp[j] > cnt_max ? cntp[j] : cnt_max;
    }
    float sp[PB], Lu[PB];
#pragma unroll
    for (int j = 0; j < PB; ++j) { sp[j] = 0.f; Lu[j] = 0.f; }
    const bool first = p0 == 0;
    // (clamped index products, not the bumped 64-bit prefetch pointers of tud_g_kernel: next to the PB recurrences those take
    // this kernel to 100 registers, one wave per SIMD fewer)
    float nxt[TUD_STAGE];
#pragma unroll
    for (int t = 0; t < TUD_STAGE; ++t) nxt[t] = od_col[(size_t)(t < nL ? t : nL - 1) * a.ld];
    for (int kc = 0; kc < nL; kc += TUD_STAGE) {
#pragma unroll
      for (int t = 0; t < TUD_STAGE; ++t) s_stage[t][threadIdx.x] = nxt[t];
#pragma unroll
      for (int t = 0; t < TUD_STAGE; ++t) nxt[t] = od_col[(size_t)(kc + TUD_STAGE + t < nL ? kc + TUD_STAGE + t : nL - 1) * a.ld];
      const int k_hi = kc + TUD_STAGE < nL ? kc + TUD_STAGE : nL;
      for (int k = kc; k < k_hi; ++k) {
        const float od = s_stage[k - kc][threadIdx.x];
#pragma unroll
        for (int j = 0; j < PB; ++j)
          if (LayerMask{mw[j][0], mw[j][1], mw[j][2], mw[j][3]}.bit(k)) sp[j] += od;
        const bool up = k < cnt_max, dn = first && down.live && k < nd;  // wave-uniform
        if (!up && !dn) continue;
        const float B = ln.planck(k);
        // per lane, the form that does not cancel (up_step). Choosing one form per pair where the whole wave agrees was
        // slower (1.48 against 1.15 ms at blocks of 4: the branches cost more than the second form)
#pragma unroll
        for (int j = 0; j < PB; ++j)
          if (k < cntp[j]) Lu[j] = up_step(Lu[j], B, od * cp[j]);
        if (dn) down.step(s_g, od, B);
      }
    }
    if (ln.live) {
#pragma unroll
      for (int j = 0; j < PB; ++j) {
        if (p0 + j < npair) {
          const size_t o = (size_t)(p0 + j) * (size_t)a.ld_out + (size_t)ln.i;
          a.tau[o] = a.return_od ? sp[j] * mup[j] : __builtin_amdgcn_exp2f(sp[j] * cp[j]);
          a.Lu[o] = Lu[j];
        }
      }
    }
  }
  if (ln.live) a.Ld[ln.i] = down.result(a);
}

// Several sensor altitudes and slant paths, the usual case of prefix masks (altitudes on an ascending height grid: the layers
// with Z <= zs are the first count(zs) ones). The reference runs the SAME upwelling recurrence for every altitude -- only the
// number of layers differs (:352-356) -- and tau's sum is then a running sum too, so one recurrence per SLANT serves every
// altitude: its value after count(zs) layers is that altitude's L-up, stored the moment the pass gets there. Cost per layer:
// Planck once + one recurrence per slant (the reference's main caller: 9 altitudes, 1 slant -- 9 passes' worth of work
// before, barely more than one now). Bit-identical to running the pairs one by one. Non-prefix masks (a height grid that is
// not ascending) take tud_g_pairs_kernel.
template <int NMU, bool PN>
__global__ __launch_bounds__(256) void tud_g_snap_kernel(TudArgs a) {
  __shared__ double s_g[TUDG_NINT * 8];
  __shared__ float s_stage[TUD_STAGE][256];  // each thread's own slots
  tudg_load(s_g, a);
  TudLane ln(a);
  const int nL = a.n_layers;
  const float* __restrict__ od_col = ln.od_col;
  float nxt[TUD_STAGE];
#pragma unroll
  for (int t = 0; t < TUD_STAGE; ++t) nxt[t] = od_col[(size_t)(t < nL ? t : nL - 1) * a.ld];
  ln.layer_consts(a);
  PlanckNodes PNd;
  if (PN) PNd = planck_nodes_setup(a, ln);
  __syncthreads();  // the table is in LDS

  const int nd = a.n_down, n_alt = a.n_alt, n_mu = a.n_mu;
  int cnt_max = 0;
  unsigned long long snap_lo = 0ull, snap_hi = 0ull;  // bit c: some altitude's column has c layers (c <= 128; 128 itself is caught at the end)
  for (int ia = 0; ia < n_alt; ++ia) {
    const int c = a.count[ia];
    cnt_max = c > cnt_max ? c : cnt_max;
    if (c < 64) snap_lo |= 1ull << c; else if (c < 128) snap_hi |= 1ull << (c - 64);
  }
  float cm[NMU], mum[NMU], Lu[NMU];
#pragma unroll
  for (int m = 0; m < NMU; ++m) { cm[m] = a.mu_c[m < n_mu ? m : 0]; mum[m] = a.mu[m < n_mu ? m : 0]; Lu[m] = 0.f; }
  float s_run = 0.f;
  TudDown down(s_g, a, ln);
  // every altitude whose column has c layers gets its outputs now
  auto snapshot = [&](int c) {
    if (c < 128 && !(((c < 64 ? snap_lo : snap_hi) >> (c & 63)) & 1ull)) return;
    for (int ia = 0; ia < n_alt; ++ia) {
      if (a.count[ia] != c || !ln.live) continue;
#pragma unroll
      for (int m = 0; m < NMU; ++m) {
        if (m < n_mu) {
          const size_t o = (size_t)(ia * n_mu + m) * (size_t)a.ld_out + (size_t)ln.i;
          a.tau[o] = a.return_od ? s_run * mum[m] : __builtin_amdgcn_exp2f(s_run * cm[m]);
          a.Lu[o] = Lu[m];
        }
      }
    }
  };
  snapshot(0);
  // as in tud_g_kernel (staged OD fetch spelled out, see there): a chunk whose layers all count for the upwelling and the downwelling runs unrolled with static
  // offsets (the layer loop is bound by the CU's one scalar unit)
  const size_t bump = (size_t)TUD_STAGE * (size_t)a.ld;
  const float* pf[TUD_STAGE];
#pragma unroll
  for (int t = 0; t < TUD_STAGE; ++t) pf[t] = od_col + (size_t)(TUD_STAGE + t) * (size_t)a.ld;
  for (int kc = 0; kc < nL; kc += TUD_STAGE) {
#pragma unroll
    for (int t = 0; t < TUD_STAGE; ++t) s_stage[t][threadIdx.x] = nxt[t];
    if (kc + 2 * TUD_STAGE <= nL) {
#pragma unroll
      for (int t = 0; t < TUD_STAGE; ++t) nxt[t] = *pf[t];
    } else {
#pragma unroll
      for (int t = 0; t < TUD_STAGE; ++t)
        if (kc + TUD_STAGE + t < nL) nxt[t] = *pf[t];
    }
#pragma unroll
    for (int t = 0; t < TUD_STAGE; ++t) pf[t] += bump;
    const int k_hi = kc + TUD_STAGE < nL ? kc + TUD_STAGE : nL;
    if (PN && k_hi == kc + TUD_STAGE && k_hi <= cnt_max && k_hi <= nd && k_hi < 64) {
      const unsigned snap_chunk = (unsigned)(snap_lo >> (kc + 1));  // bit t: some altitude's column ends after layer kc + t
#pragma unroll
      for (int t = 0; t < TUD_STAGE; ++t) {
        const float od = s_stage[t][threadIdx.x];
        const float B = planck_nodes_eval(PNd, false, kc + t);  // kc + t < 64
        s_run += od;
#pragma unroll
        for (int m = 0; m < NMU; ++m)
          if (NMU == 1 || m < n_mu) Lu[m] = up_step(Lu[m], B, od * cm[m]);
        if ((snap_chunk >> t) & 1u) snapshot(kc + t + 1);
        if (down.live) down.step(s_g, od, B);
      }
      continue;
    }
    for (int k = kc; k < k_hi; ++k) {
      const float od = s_stage[k - kc][threadIdx.x];
      const bool up = k < cnt_max, dn = down.live && k < nd;  // wave-uniform
      if (!up && !dn) continue;
      const float B = PN ? planck_nodes_eval(PNd, k) : ln.planck(k);
      if (up) {
        s_run += od;
#pragma unroll
        for (int m = 0; m < NMU; ++m)
          if (m < n_mu) Lu[m] = up_step(Lu[m], B, od * cm[m]);
        snapshot(k + 1);
      }
      if (dn) down.step(s_g, od, B);
    }
  }
  if (ln.live) a.Ld[ln.i] = down.result(a);
}

// Host side of G: piecewise Chebyshev interpolants of degree TUDG_DEG in fp64, stored as monomials in (S - mid).
static void tudg_build(int n_angle, std::vector<double>& tab, double& g0_out) {
  const TudQuadrature quad = tud_quadrature(n_angle);
  std::vector<double> sec;
  for (int ii = 1; ii < n_angle; ++ii) sec.push_back(1.0 / cos(quad.th[ii]));  // theta = 0 has weight exactly 0
  auto G = [&](double S) { double r = 0.0; for (size_t q = 0; q < sec.size(); ++q) r += quad.w[q + 1] * exp(-S * sec[q]); return r; };
  constexpr int N = TUDG_DEG + 1;
  tab.assign((size_t)TUDG_NINT * 8, 0.0);
  for (int idx = 0; idx < TUDG_NINT; ++idx) {
    double lo, hi;
    if (idx < TUDG_NLOG) {
      union { int i; float f; } a0, a1;
      a0.i = (TUDG_BASE + idx) << (23 - TUDG_M);
      a1.i = (TUDG_BASE + idx + 1) << (23 - TUDG_M);
      lo = (double)a0.f - (double)TUDG_OFF;
      hi = (double)a1.f - (double)TUDG_OFF;
      if (lo < 0.0) lo = 0.0;
      if (hi > (double)TUDG_SWITCH) hi = (double)TUDG_SWITCH;
    } else {
      lo = (double)TUDG_SWITCH + 0.5 * (idx - TUDG_NLOG);
      hi = lo + 0.5;
    }
    const double mid = 0.5 * (lo + hi), hw = 0.5 * (hi - lo) * 1.002;  // a little wider than the bucket: (float)S rounds at the edges
    double y[N], c[N];
    for (int k = 0; k < N; ++k) y[k] = G(mid + hw * cos(M_PI * (k + 0.5) / N));
    for (int j = 0; j < N; ++j) {
      double sacc = 0.0;
      for (int k = 0; k < N; ++k) sacc += y[k] * cos(M_PI * j * (k + 0.5) / N);
      c[j] = sacc * (j == 0 ? 1.0 : 2.0) / N;
    }
    // Chebyshev -> monomials in t = u / hw:  T0 = 1, T1 = t, T_{n+1} = 2 t T_n - T_{n-1}
    double mono[N] = {0}, Tm[N] = {0}, Tc[N] = {0}, Tn[N];
    Tm[0] = 1.0;  // T0
    Tc[1] = 1.0;  // T1
    mono[0] += c[0];
    if (N > 1) mono[1] += c[1];
    for (int n = 2; n < N; ++n) {
      for (int d = 0; d < N; ++d) Tn[d] = (d > 0 ? 2.0 * Tc[d - 1] : 0.0) - Tm[d];
      for (int d = 0; d < N; ++d) { mono[d] += c[n] * Tn[d]; Tm[d] = Tc[d]; Tc[d] = Tn[d]; }
    }
    double* row = &tab[(size_t)idx * 8];
    row[0] = mid;
    double sc = 1.0;
    for (int d = 0; d < N; ++d) { row[1 + d] = mono[d] * sc; sc /= hw; }
  }
  g0_out = quad.wsum;  // G(0)
}

// The table as the kernels see it, for host-side checks (tests/test_host.py evaluates it in NumPy against the direct sum;
// no device involved): table_h [rtx_tud_gtable_size()] doubles = TUDG_NINT rows of {interval centre, a0 .. a6}.
extern "C" int rtx_tud_gtable_size(void) { return TUDG_NINT * 8; }
extern "C" int rtx_tud_gtable(int n_angle, double* table_h, double* g0_h) {
  if (n_angle < 1 || n_angle > TUD_MAX_ANGLES - 32) RTX_FAIL("n_angle=%d outside [1,%d]", n_angle, TUD_MAX_ANGLES - 32);
  if (!table_h || !g0_h) RTX_FAIL("a required pointer is NULL");
  std::vector<double> tab;
  tudg_build(n_angle, tab, *g0_h);
  memcpy(table_h, tab.data(), tab.size() * sizeof(double));
  return 0;
}

// tud_g_kernel's early launch: a depth S that no downwelling which has stopped looking can lie below. It stops at G(S) <=
// G(0) 2^-min(opaque_y, 120) with opaque_y >= 27; G falls monotonically, so S exceeds the root of G(S) = G(0) 2^-26.5 (half a
// binade of margin against the table's 4e-14 G(0)), found by bisection on the direct sum; 1e-4 off for the kernel's fp32
// sum of the chunk. One value per n_angle, kept.
static float tudg_early_smin(int n_angle) {
  static std::mutex mu;
  static std::map<int, float> memo;
  std::lock_guard<std::mutex> lock(mu);
  auto it = memo.find(n_angle);
  if (it != memo.end()) return it->second;
  const TudQuadrature quad = tud_quadrature(n_angle);
  float r = -INFINITY;
  if (n_angle > 1 && quad.wsum > 0.0) {
    auto G = [&](double S) { double g = 0.0; for (int ii = 1; ii < n_angle; ++ii) g += quad.w[ii] * exp(-S / cos(quad.th[ii])); return g; };
    const double target = quad.wsum * exp2(-26.5);
    double lo = 0.0, hi = TUDG_SMAX;
    if (G(hi) < target) {
      for (int it2 = 0; it2 < 60; ++it2) { const double mid = 0.5 * (lo + hi); (G(mid) > target ? lo : hi) = mid; }
      r = (float)(lo * (1.0 - 1e-4));
    }
  }
  memo[n_angle] = r;
  return r;
}

// The device copy of the table, one per (device, n_angle), never forgotten.
static int tudg_table(int n_angle, DevTableCache<double>::Hit* out) {
  static DevTableCache<double>* const cache = new DevTableCache<double>(0);
  int dev = 0;
  RTX_HIP(hipGetDevice(&dev));
  return cache->get(dev, &n_angle, sizeof(n_angle), [&](std::vector<double>& tab) { double g0; tudg_build(n_angle, tab, g0); return 0; }, out);
}

// one thread per wavenumber of the shard, 256 per workgroup
static int tud_launch(void (*kernel)(TudArgs), const TudArgs& a, size_t lds_bytes, hipStream_t st) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)((a.g.n + 255) / 256)), dim3(256), lds_bytes, st, a);
  RTX_LAUNCH_CHECK();
  return 0;
}

template <int NA>
static int launch_tud(TudArgs& a, int na, hipStream_t st) {
  const int na_pad = na == 0 ? NA : ((na + NA - 1) / NA) * NA;  // at least one block: it carries tau and L-up
  float cmin = (float)LOG2E, cmax = (float)LOG2E;
  for (int q = 0; q < na; ++q) { cmin = q == 0 ? -a.ang_c[q] : fminf(cmin, -a.ang_c[q]); cmax = q == 0 ? -a.ang_c[q] : fmaxf(cmax, -a.ang_c[q]); }
  // pads: weight-0 copies of the last stream (keeps |c| ascending with the stream index, which the per-block form
  // selection of mixed layers relies on); with no stream at all, nadir
  for (int q = na; q < na_pad; ++q) { a.ang_c[q] = na > 0 ? a.ang_c[na - 1] : (float)(-LOG2E); a.ang_w[q] = 0.f; }
  a.ang_cmin = cmin; a.ang_cmax = cmax;
  a.n_ang = na_pad;
  if (a.n_layers <= TUD_COL_LAYERS) return tud_launch(tud_kernel<NA, true>, a, (size_t)a.n_layers * 256 * sizeof(float), st);
  return tud_launch(tud_kernel<NA, false>, a, (size_t)TUD_STAGE * 256 * sizeof(float), st);
}

// RADTXFR_TUD_KERNEL=streams forces the stream kernel (cross-checks and timing); RADTXFR_TUD_SKIP=0 keeps every wave of
// tud_g_kernel on the full pass. Each read once.
static bool tud_force_streams() {
  static int v = -1;
  if (v < 0) { const char* e = getenv("RADTXFR_TUD_KERNEL"); v = (e && !strcmp(e, "streams")) ? 1 : 0; }
  return v != 0;
}
static bool tud_skip_on() {
  static int v = -1;
  if (v < 0) { const char* e = getenv("RADTXFR_TUD_SKIP"); v = (e && !strcmp(e, "0")) ? 0 : 1; }
  return v != 0;
}
// B_k across a wave by a parabola through three of its wavenumbers (PlanckNodes) where that is exact to 1e-10:
// |d ln B / d nu| <= 4/nu + c2/T, and the parabola's error is 0.008 (that x 63 steps)^3
// decided on the FULL axis (its lowest wavenumber is the worst case), so that every wavenumber shard runs the
// instantiation the single-rank run does; a shard offset that is a multiple of 64 then has the same waves, hence bits
static bool tud_planck_nodes(const rtx_grid* grid, double t_min) {
  const double nu_lo = grid->xmin;
  return nu_lo > 0.0 && (4.0 / nu_lo + RT_C2 * 100.0 / t_min) * 63.0 * grid->step <= 7e-3;
}

// phase 0: the whole pass in one launch. 1 / 2: tud_g_kernel<true, true>'s early / late launch with the flags of `done`
// (one byte per 64 points, padded to whole workgroups); the caller has checked with tud_split_layers() that this call
// launches that instantiation.
static int tud_opts_impl(const float* OD, int64_t ld, const rtx_grid* grid, int n_layers, const double* T_h, int n_alt,
                         const uint8_t* mask_h, int n_mu, const double* mu_h, int n_down, int n_angle, int return_od,
                         float* tau, float* Lu, float* Ld, float* Ld_angles, int64_t ld_out, void* stream, unsigned flags,
                         int phase, unsigned char* done) {
  if (rtx_check_grid(grid)) return 1;
  if (flags & ~(unsigned)RTX_TUD_OD_NONNEG) RTX_FAIL("flags=0x%x: unknown bits", flags);
  if (!OD || !T_h || !mask_h || !mu_h || !tau || !Lu || !Ld) RTX_FAIL("a required pointer is NULL");
  if (n_layers < 1 || n_layers > TUD_MAX_LAYERS) RTX_FAIL("n_layers=%d outside [1,%d]", n_layers, TUD_MAX_LAYERS);
  if (n_alt < 1 || n_alt > TUD_MAX_ALT) RTX_FAIL("n_alt=%d outside [1,%d]", n_alt, TUD_MAX_ALT);
  if (n_mu < 1 || n_mu > TUD_MAX_MU) RTX_FAIL("n_mu=%d outside [1,%d]", n_mu, TUD_MAX_MU);
  if (n_angle < 1 || n_angle > TUD_MAX_ANGLES - 32) RTX_FAIL("n_angle=%d outside [1,%d]", n_angle, TUD_MAX_ANGLES - 32);
  if (n_down < 0 || n_down > n_layers) RTX_FAIL("n_down=%d outside [0,%d]", n_down, n_layers);
  if (ld < grid->n || ld_out < grid->n) RTX_FAIL("leading dimension smaller than the shard");
  if (grid->n == 0) return 0;
  TudArgs a;
  memset(&a, 0, sizeof(a));
  a.OD = OD; a.ld = ld; a.ld_out = ld_out; a.g = to_dev(grid);
  a.n_layers = n_layers; a.n_alt = n_alt; a.n_mu = n_mu; a.n_down = n_down; a.return_od = return_od;
  a.tau = tau; a.Lu = Lu; a.Ld = Ld; a.Ld_ang = Ld_angles;
  if (tud_layer_consts(T_h, n_layers, a.c2l2e_over_T)) return 1;
  double t_max = T_h[0], t_min = T_h[0];
  for (int k = 1; k < n_layers; ++k) {
    if (T_h[k] > t_max) t_max = T_h[k];
    if (T_h[k] < t_min) t_min = T_h[k];
  }
  a.c2l2e_over_Tmax = c2l2e_over(t_max);
  a.c2l2e_over_Tmin = c2l2e_over(t_min);
  for (int ia = 0; ia < n_alt; ++ia) {
    int c = 0;
    for (int k = 0; k < n_layers; ++k)
      if (mask_h[(size_t)ia * n_layers + k]) { a.mask[ia][k >> 5] |= 1u << (k & 31); ++c; }
    a.count[ia] = c;
  }
  for (int m = 0; m < n_mu; ++m) { a.mu[m] = (float)mu_h[m]; a.mu_c[m] = (float)(-LOG2E * mu_h[m]); }
  // theta=0 has weight exactly 0 (sin 0 = 0) and is skipped; an odd count is padded with a weight-0 stream.
  const TudQuadrature quad = tud_quadrature(n_angle);
  int na = 0;
  for (int ii = Ld_angles ? 0 : 1; ii < n_angle; ++ii) {  // with per-stream output every stream is evaluated
    a.ang_c[na] = (float)(-LOG2E / cos(quad.th[ii]));
    a.ang_w[na] = (float)quad.w[ii];
    ++na;
  }
  a.n_ang_real = na;
  a.inv_wsum = (float)(1.0 / quad.wsum);  // n_angle==1: 1/0 = inf, acc=0 -> NaN like the reference's 0/0
  if (na == 0) a.inv_wsum = NAN;
  // streams per register block: the smallest instantiated width that holds them all (N_angle = 30 -> 29
  // evaluated -> 29 registers, no padding); more than 32 streams run in blocks of 32
  hipStream_t st = (hipStream_t)stream;
  // default: the angle-summed form; the stream kernel when the caller wants the per-stream radiances
  // (RADTXFR_TUD_KERNEL=streams forces it, for cross-checks and timing)
  const bool force_streams = tud_force_streams();
  if (phase != 0 && (Ld_angles || force_streams)) RTX_FAIL("internal: a two-launch pass without tud_g_kernel");
  if (!Ld_angles && !force_streams) {
    DevTableCache<double>::Hit gt;  // with the cache's lock, held until the launch below has returned
    if (tudg_table(n_angle, &gt)) return 1;
    a.gtab = gt.d; a.g0 = quad.wsum;  // G(0)
    bool prefix = true;  // every altitude's mask = its first count layers?
    for (int ia = 0; ia < n_alt && prefix; ++ia)
      for (int k = 0; k < n_layers; ++k)
        if ((mask_h[(size_t)ia * n_layers + k] != 0) != (k < a.count[ia])) { prefix = false; break; }
    const bool pn = tud_planck_nodes(grid, t_min);  // B_k across a wave by a parabola where that is exact to 1e-10
    void (*kernel)(TudArgs);
    if (phase != 0 && n_alt * n_mu != 1) RTX_FAIL("internal: a two-launch pass with more than one pair");
    if (n_alt * n_mu == 1) {
      kernel = pn ? tud_g_kernel<true, false> : tud_g_kernel<false, false>;
      // hidden layers of an opaque column (see the kernel): RADTXFR_TUD_SKIP=0 keeps every wave on the full pass
      a.skip = tud_skip_on() && (flags & RTX_TUD_OD_NONNEG) && !return_od && prefix && pn;  // (the Planck-node instantiation only)
      if (a.skip) kernel = tud_g_kernel<true, true>;  // every other call runs the instantiation without the look
      if (phase != 0) {
        if (!a.skip || !done) RTX_FAIL("internal: a two-launch pass without the look at the top");
        a.done = done;
        a.early_smin = n_down >= TUD_STAGE ? tudg_early_smin(n_angle) : -INFINITY;
        kernel = phase == 1 ? tud_g_kernel<true, true, 1> : tud_g_kernel<true, true, 2>;
      }
    }
    // one slant path (the reference's main caller: 9 altitudes, nadir): the instantiation without the per-slant guards
    else if (prefix && n_mu == 1) kernel = pn ? tud_g_snap_kernel<1, true> : tud_g_snap_kernel<1, false>;
    else if (prefix) kernel = pn ? tud_g_snap_kernel<TUD_MAX_MU, true> : tud_g_snap_kernel<TUD_MAX_MU, false>;
    else kernel = tud_g_pairs_kernel<TUDG_PB>;
    return tud_launch(kernel, a, 0, st);
  }
  if (na <= 4) return launch_tud<4>(a, na, st);
  if (na <= 8) return launch_tud<8>(a, na, st);
  if (na <= 16) return launch_tud<16>(a, na, st);
  if (na <= 24) return launch_tud<24>(a, na, st);
  if (na <= 29) return launch_tud<29>(a, na, st);
  return launch_tud<32>(a, na, st);
}

extern "C" int rtx_tud_opts(const float* OD, int64_t ld, const rtx_grid* grid, int n_layers, const double* T_h, int n_alt,
                            const uint8_t* mask_h, int n_mu, const double* mu_h, int n_down, int n_angle, int return_od,
                            float* tau, float* Lu, float* Ld, float* Ld_angles, int64_t ld_out, void* stream, unsigned flags) {
  return tud_opts_impl(OD, ld, grid, n_layers, T_h, n_alt, mask_h, n_mu, mu_h, n_down, n_angle, return_od, tau, Lu, Ld, Ld_angles,
                       ld_out, stream, flags, 0, nullptr);
}

extern "C" int rtx_tud(const float* OD, int64_t ld, const rtx_grid* grid, int n_layers, const double* T_h, int n_alt,
                       const uint8_t* mask_h, int n_mu, const double* mu_h, int n_down, int n_angle, int return_od,
                       float* tau, float* Lu, float* Ld, float* Ld_angles, int64_t ld_out, void* stream) {
  return rtx_tud_opts(OD, ld, grid, n_layers, T_h, n_alt, mask_h, n_mu, mu_h, n_down, n_angle, return_od, tau, Lu, Ld, Ld_angles,
                      ld_out, stream, 0u);
}

// ---------------------------------------------------------------------------------------------------
// compute_TUD in one call (radiative_transfer.py:274-392 with compute_OD := the Voigt line-sum): prologue, line-sum and
// TUD integration enqueued back to back. Same kernels as the three separate entry points; what it saves is host time per
// atmosphere (one FFI crossing, no per-call Python marshalling between the stages), which is what limits a wavenumber
// shard small enough to finish in a few hundred microseconds (8-GPU strong scaling, tools/time_overhead.py).
// The layers the two-launch pass sums first and last, if this call may take it (rtx_compute_tud_opts): the TUD step would
// launch tud_g_kernel<true, true> -- exactly tud_opts_impl's conditions, restated on the host arguments before anything is
// enqueued -- and there is a chunk to leave out between the bottom chunk and the look at the top. k_mid0 / k_mid1: the
// middle layers [k_mid0, k_mid1). Arguments that tud_opts_impl would refuse give false: the plain order reports them.
static bool tud_split_layers(const rtx_grid* grid, int n_layers, const double* T_h, int n_alt, const uint8_t* mask_h, int n_mu,
                             int return_od, unsigned tud_flags, int* k_mid0, int* k_mid1) {
  if (!tud_skip_on() || tud_force_streams() || !(tud_flags & RTX_TUD_OD_NONNEG) || return_od) return false;
  if (!grid || !T_h || !mask_h || n_alt != 1 || n_mu != 1 || n_layers < 1 || n_layers > TUD_MAX_LAYERS) return false;
  int cnt0 = 0;
  for (int k = 0; k < n_layers; ++k) cnt0 += mask_h[k] != 0;
  for (int k = 0; k < n_layers; ++k)
    if ((mask_h[k] != 0) != (k < cnt0)) return false;  // not a prefix mask
  double t_min = T_h[0];
  for (int k = 1; k < n_layers; ++k) t_min = T_h[k] < t_min ? T_h[k] : t_min;
  if (!tud_planck_nodes(grid, t_min)) return false;
  if (cnt0 < 1) return false;
  const int k_top = (cnt0 - 1) & ~(TUD_STAGE - 1);
  const int k_deep = k_top - (TUD_SKIP_SCAN - TUD_STAGE);  // the lowest layer the look at the top can read
  if (TUD_SKIP_BOTTOM + TUD_STAGE > k_deep) return false;
  *k_mid0 = TUD_SKIP_BOTTOM; *k_mid1 = k_deep;
  return true;
}

// RADTXFR_OD_SKIP=0: rtx_compute_tud_opts keeps the plain order (one line-sum over all layers, one TUD launch) whatever its
// flags say -- for A/B timing and for support. Read once.
static bool od_skip_on() {
  static int v = -1;
  if (v < 0) { const char* e = getenv("RADTXFR_OD_SKIP"); v = (e && !strcmp(e, "0")) ? 0 : 1; }
  return v != 0;
}

// RTX_CTUD_OD_SCRATCH, where the call is eligible (include/radtxfr_hip.h):
//   prologue -> tile ranges -> line-sum A: layers [0, TUD_SKIP_BOTTOM) and [k_top - (TUD_SKIP_SCAN - TUD_STAGE), n_layers)
//            -> TUD early: the waves that need nothing else finish and say so (tud_g_kernel, PHASE 1)
//            -> line-sum B: the layers in between, without the rows of those waves; a tile whose 16 rows are all done returns at once
//            -> TUD late: every other wave (PHASE 2)
// On the C3 column the layers of B are the low, wide-winged ones, and a third of the tiles are hidden whole.
extern "C" int rtx_compute_tud_opts(rtx_prep* prep, const rtx_lines* lines, const rtx_grid* grid, int n_layers, const double* T_h,
                                    const double* p_atm_h, const double* qratio_h, const double* weight_h, const double* mass_h,
                                    double dil_air, double dil_self, double omega_wing, double omega_wing_hw,
                                    double intensity_threshold, int n_alt, const uint8_t* mask_h, int n_mu, const double* mu_h,
                                    int n_down, int n_angle, int return_od, float* OD, int64_t ld_od, float* tau, float* Lu,
                                    float* Ld, int64_t ld_out, void* stream, unsigned flags) {
  if (flags & ~(unsigned)RTX_CTUD_OD_SCRATCH) RTX_FAIL("flags=0x%x: unknown bits", flags);
  if (!OD) RTX_FAIL("OD workspace is NULL");
  if (rtx_line_prep_profile(prep, lines, grid, n_layers, T_h, p_atm_h, qratio_h, weight_h, mass_h, dil_air, dil_self, omega_wing,
                            omega_wing_hw, intensity_threshold, 1.0, RTX_PROFILE_VOIGT, stream))
    return 1;
  // the optical depths are sums of non-negative terms when every factor the caller gave is finite and >= 0: the
  // column weights, the partition-sum ratios, T and p (the prologue has accepted lines, n_layers and the arrays by now). Line
  // strengths are the table's and are not looked at: a table with a negative or NaN S is outside what this vouches for.
  auto nonneg = [](const double* v, long long n) {
    for (long long j = 0; j < n; ++j)
      if (!(v[j] >= 0.0 && v[j] <= 1.7976931348623157e308)) return false;
    return true;
  };
  const long long n_sl = (long long)lines->n_species * n_layers;
  const unsigned tud_flags = nonneg(weight_h, n_sl) && nonneg(qratio_h, n_sl) && nonneg(T_h, n_layers) && nonneg(p_atm_h, n_layers)
                                 ? RTX_TUD_OD_NONNEG : 0u;
  int k_mid0 = 0, k_mid1 = 0;
  if ((flags & RTX_CTUD_OD_SCRATCH) && od_skip_on() && grid->n > 0 && rtx_voigt_layers_ok(prep) &&
      tud_split_layers(grid, n_layers, T_h, n_alt, mask_h, n_mu, return_od, tud_flags, &k_mid0, &k_mid1)) {
    const size_t n_done = (size_t)((grid->n + 1023) / 1024) * 16;  // whole line-sum tiles (hence whole TUD workgroups of 4 waves)
    if (rtx_voigt_tile_points() != 1024) RTX_FAIL("internal: the done flags are laid out for tiles of 16 rows of 64 points");
    if (prep->done.reserve(n_done)) return 1;
    unsigned char* done = prep->done.get();
    const VoigtLayers la{k_mid0, 0, k_mid1, k_mid0 + (n_layers - k_mid1), nullptr, true};
    const VoigtLayers lb{k_mid1 - k_mid0, k_mid0, 0, k_mid1 - k_mid0, done, false};
    if (rtx_voigt_sum_layers(prep, grid, n_layers, OD, ld_od, stream, la)) return 1;
    if (tud_opts_impl(OD, ld_od, grid, n_layers, T_h, n_alt, mask_h, n_mu, mu_h, n_down, n_angle, return_od, tau, Lu, Ld, nullptr,
                      ld_out, stream, tud_flags, 1, done))
      return 1;
    if (rtx_voigt_sum_layers(prep, grid, n_layers, OD, ld_od, stream, lb)) return 1;
    return tud_opts_impl(OD, ld_od, grid, n_layers, T_h, n_alt, mask_h, n_mu, mu_h, n_down, n_angle, return_od, tau, Lu, Ld, nullptr,
                         ld_out, stream, tud_flags, 2, done);
  }
  if (rtx_voigt_sum(prep, grid, n_layers, OD, nullptr, ld_od, stream)) return 1;
  return rtx_tud_opts(OD, ld_od, grid, n_layers, T_h, n_alt, mask_h, n_mu, mu_h, n_down, n_angle, return_od, tau, Lu, Ld, nullptr,
                      ld_out, stream, tud_flags);
}

extern "C" int rtx_compute_tud(rtx_prep* prep, const rtx_lines* lines, const rtx_grid* grid, int n_layers, const double* T_h,
                               const double* p_atm_h, const double* qratio_h, const double* weight_h, const double* mass_h,
                               double dil_air, double dil_self, double omega_wing, double omega_wing_hw,
                               double intensity_threshold, int n_alt, const uint8_t* mask_h, int n_mu, const double* mu_h,
                               int n_down, int n_angle, int return_od, float* OD, int64_t ld_od, float* tau, float* Lu,
                               float* Ld, int64_t ld_out, void* stream) {
  return rtx_compute_tud_opts(prep, lines, grid, n_layers, T_h, p_atm_h, qratio_h, weight_h, mass_h, dil_air, dil_self, omega_wing,
                              omega_wing_hw, intensity_threshold, n_alt, mask_h, n_mu, mu_h, n_down, n_angle, return_od, OD, ld_od,
                              tau, Lu, Ld, ld_out, stream, 0u);
}
