// Internal definitions shared by the HIP translation units of libradtxfr_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/radtxfr_hip.h"
#include "rtx_devmem.h"

// ---- error plumbing (thread-local text behind rtx_last_error) ---------------------------------
void rtx_set_error(const char* fmt, ...);
#define RTX_FAIL(...)          \
  do {                         \
    rtx_set_error(__VA_ARGS__); \
    return 1;                  \
  } while (0)
#define RTX_HIP(call)                                                                        \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) RTX_FAIL("%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
  } while (0)
#define RTX_LAUNCH_CHECK()                                                                   \
  do {                                                                                       \
    hipError_t e_ = hipGetLastError();                                                       \
    if (e_ != hipSuccess) RTX_FAIL("%s:%d kernel launch -> %s", __FILE__, __LINE__, hipGetErrorString(e_)); \
  } while (0)

// ---- device-side view of the spectral grid ------------------------------------------------------
struct GridDev {
  double xmin, xmax, step;
  long long n_total, offset, n;
};
static inline GridDev to_dev(const rtx_grid* g) {
  GridDev d;
  d.xmin = g->xmin; d.xmax = g->xmax; d.step = g->step;
  d.n_total = g->n_total; d.offset = g->offset; d.n = g->n;
  return d;
}
int rtx_check_grid(const rtx_grid* g);

// X[ig] for a GLOBAL index exactly as np.linspace builds it: arange*step + start (two roundings,
// never fused), last point pinned to xmax. Indices outside [0,n_total) extrapolate.
__device__ __forceinline__ double grid_x(const GridDev& g, long long ig) {
  double v = __dadd_rn(__dmul_rn((double)ig, g.step), g.xmin);
  return (ig == g.n_total - 1) ? g.xmax : v;
}

// ---- XCD-aware tile order of the line-sum kernels ------------------------------------------------
// Workgroup b runs on XCD b & 7 (round-robin dispatch). An XCD walks chunks of RTX_XCD_CHUNK consecutive tiles, so
// neighbouring tiles share their line records in that XCD's L2; the chunks are dealt round-robin over the XCDs, so
// every XCD sees the whole spectrum. (One contiguous eighth of the spectrum per XCD left the XCD with the highest
// wavenumbers -- widest Doppler cores, most Weideman rows -- as the straggler of every launch.)
#ifndef RTX_XCD_CHUNK
#define RTX_XCD_CHUNK 16
#endif
__device__ __forceinline__ int xcd_tile(int b) {
  const int idx = b >> 3, c = idx / RTX_XCD_CHUNK, w = idx - c * RTX_XCD_CHUNK;
  return (c * 8 + (b & 7)) * RTX_XCD_CHUNK + w;
}
static inline int xcd_slots(int n_tiles) {  // block slots per XCD: grid.x = 8 * xcd_slots(n_tiles)
  const int n_chunks = (n_tiles + RTX_XCD_CHUNK - 1) / RTX_XCD_CHUNK;
  return ((n_chunks + 7) / 8) * RTX_XCD_CHUNK;
}

// ---- Planck radiance in fp32 from an fp64 exponent (shared by the TUD and at-sensor kernels) ----------
#define RT_C1 1.19104295315e-16  // radiative_transfer.py:71
#define RT_C2 1.43877736830e-02  // radiative_transfer.py:72
#define LOG2E 1.4426950408889634
#define LN2 0.6931471805599453
// B(nu,T) in uW/(cm^2 sr cm^-1):  c1*(100 nu)^3*1e4 / (exp(c2*100 nu/T) - 1)
__device__ __forceinline__ float planck_f32(double c1x3, double x, double c2l2e_over_T) {
  const double t = x * c2l2e_over_T;  // log2 of the exponential, fp64
  if (t < 1.5) {                      // small arguments (far-IR / microwave): expm1 in fp64
    return (float)(c1x3 / expm1(t * LN2));
  }
  const double n = rint(t);
  const float f = (float)(t - n);     // |f| <= 1/2, exact difference
  const float e = ldexpf(__builtin_amdgcn_exp2f(f), (int)n);  // inf above 2^128: B -> 0, as it should
  return (float)c1x3 * __builtin_amdgcn_rcpf(e - 1.0f);
}

// ---- per-(line,layer) records written by the prologue, read by the line-sum --------------------
// fp32 record (48 B): everything the asymptotic (far-wing) evaluation needs, relative to the grid.
// x(i) = (i - i0)*a + c ;  contribution = (xx*Ay + Ay0) / ((xx + b1)*xx + b0),  xx = x*x.
struct __attribute__((aligned(16))) LineRec {
  float a;    // x per grid index = step*cte,  cte = sqrt(ln2)/GammaD
  float c;    // x at grid index i0            = (X[i0]-nu0')*cte
  float b1;   // 2y^2 - 1,        y = Gamma0*cte
  float b0;   // (y^2 + 1/2)^2
  float Ay;   // A*y/sqrt(pi)
  float Ay0;  // Ay*(y^2 + 1/2)
  float y;    // for the fp32 Weideman branch
  float A;    // weight*S(T)*cte/sqrt(pi)*scale  (strength times the profile's prefactor)
  int i0;     // LOCAL grid index nearest to the shifted centre nu0' (may lie outside [0,n))
  int lo;     // window = local indices [lo,hi): bisect(X,nu0-W), bisect(X,nu0+W) clipped to the shard
  int hi;
  int zw;     // half-width, in grid points, of the band around i0 that can hold |x|+y<15 (0: none)
};
// On an explicit axis (rtx_line_prep_axis / voigt_axis_kernel) the grid-relative fields take axis meanings: a = (float)cte,
// c = 0 (unused: x is formed per tile from the fp64 record, rtx_voigt_axis.hip), lo / hi = the window as axis indices
// (bisect_right), and [i0, zw) = the axis indices that can hold |x|+y<15 (empty when zw <= i0).
// fp64 companion (32 B), read only where the Weideman region is entered.
struct __attribute__((aligned(16))) LineRec64 {
  double sg0;  // nu0 + Shift0
  double cte;
  double y;
  double A;
};

// fp64 record of the speed-dependent Voigt sum (rtx_sdvoigt_sum): PROFILE_SDVOIGT's arguments (misc/hapi.py:10897)
// and the line's weight * S(T).
struct __attribute__((aligned(16))) LineRecSD {
  double nu, cte, Gam0, Shift0, Gam2, WS;
  double inv_Gam2, csqrtY;  // 1 / Gam2 and 1 / (2 cte Gam2): per-line reciprocals the line-sum would otherwise redo per point
};

// Temperature-derivative records of rtx_line_prep_dt, one pair per (line, layer), read by rtx_voigt_sum_dt beside the
// line's LineRec / LineRec64. With g = A K(x, y) the line's contribution at a point,
//   dg/dT = A [alpha K + K_x x' + K_y y'],  x' = -sx - x h,  y' = gy - y h.
// fp64 record (32 B): what the band lanes (|x| + y < 15) combine with the complex probability function in fp64.
struct __attribute__((aligned(16))) LineRecDT64 {
  double alpha;  // dlnS/dT + dlnw/dT - 1/(2T)
  double sx;     // Shift0' cte
  double gy;     // Gamma0' cte
  double h;      // 1/(2T)
};
// fp32 record (32 B): the far-wing derivative as a rational in x and xx = x*x. With p = yh - xx, q = y2 x and
// R = (xx + b1) xx + b0 (LineRec) = p^2 + q^2:
//   dg/dT = Ap / R * [ alpha y (yh + xx) + q (2 p / R - 1) x' + ((p^2 - q^2) / R - p) yp ].
struct __attribute__((aligned(16))) LineRecDT {
  float alpha, sx, yp, h;  // yp = y' = gy - y h
  float Ap;                // A / sqrt(pi)
  float yh;                // y^2 + 1/2
  float y2;                // 2 y
  float y;
};

struct rtx_lines {
  long long n = 0;
  int n_species = 0;
  DevBuf<double> nu, sw, elower, gamma_air, gamma_self, n_air, n_self, delta_air, deltap_air, delta_self;
  DevBuf<double> sd_air, sd_self;  // optional speed-dependence columns (rtx_lines_set_sd), empty = 0
  DevBuf<double> deltap_self;      // optional (rtx_lines_set_deltap_self), empty = 0
  DevBuf<double> zn;               // per line: exp(-c2 E''/Tref) (1 - exp(-c2 nu/Tref)), the layer-independent half of S(T), formed once at creation
  DevBuf<int> species;
  // host side, for the bound on candidates per tile (hot-tile split, below): the sorted centres and column extremes
  std::vector<double> nu_host;
  double ga_max = 0.0, gs_max = 0.0, n_lo = 1e300, n_hi = -1e300;
  double na_lo = 1e300, na_hi = -1e300, ns_lo = 1e300, ns_hi = -1e300;  // n ranges of the air and the self column sets on their own (self after its n_air fallback)
  // extra broadener column sets (rtx_lines_set_broadeners): [n_extra][n] each, every column filled (absent gamma / delta /
  // deltap / SD = 0, absent n = n_air), so the mixed prologue reads them without tests
  int n_extra = 0;
  DevBuf<double> x_gamma, x_n, x_delta, x_deltap, x_sd;
  std::vector<double> x_gmax, x_nlo, x_nhi;  // host, [n_extra]: |gamma| maximum and n range of each set (hot-tile bound)
  // Hartmann-Tran columns (rtx_lines_set_ht): the columns given, [n_cols][n], and per column set (0 air, 1 self, 2 + j) the
  // device pointers of its RTX_HT_COLS slots, [2 + RTX_MAX_BROADENERS][RTX_HT_COLS] (NULL: absent); empty = no HT column
  DevBuf<double> ht_data;
  DevBuf<const double*> ht_ptr;
};

// ---- hot tiles ---------------------------------------------------------------------------------------
// Real line lists cluster (band heads: thousands of lines inside a cm^-1), and one line-sum workgroup per (tile, layer)
// then serialises the launch on its few hot tiles (the clustered synthetic table: slowest workgroup = 2x the ideal
// duration of the whole launch, tools/tile_spread.py). A tile with more than RTX_SPLIT_MIN candidates is therefore cut
// into parts of RTX_SPLIT_PART consecutive candidates: part 0 stays with the tile's own workgroup, every further part is
// an item of a work list (written by tile_ranges_kernel) that extra workgroups evaluate into a workspace of partial
// tiles, and a last kernel adds a tile's parts to its optical depths in part order. The cut is a function of the
// (canonical) candidate range alone, so results stay bit-reproducible and independent of how the axis is sharded.
#ifndef RTX_SPLIT_PART
#define RTX_SPLIT_PART 256  // candidates per part (clustered C3 table, prologue + line-sum: 512 -> 2.83 ms, 256 -> 2.57, 128 -> 2.83; unsplit 5.47)
#endif
#ifndef RTX_SPLIT_MIN
#define RTX_SPLIT_MIN 768   // tiles with more candidates than this are cut: three times a part, so that the ~100-300 candidates of an ordinary tile never are
#endif
struct __attribute__((aligned(16))) SplitItem {
  int tile, k;    // tile of the shard, layer
  int lo, hi;     // candidate slots [lo, hi)
  int part;       // 1 .. extra
  int extra;      // number of extra parts of this (tile, layer); its items are consecutive, part 1 first
  int pad0, pad1;
};

struct rtx_prep {
  long long n_lines = 0;
  int max_layers = 0;
  int n_layers = 0;           // of the last rtx_line_prep
  DevBuf<LineRec> rec;        // [max_layers][n_lines]
  DevBuf<LineRec64> rec64;    // [max_layers][n_lines]
  DevBuf<int> ic;             // [n_lines] local grid index nearest the UNSHIFTED centre (sorted)
  DevBuf<int2> win;           // [max_layers][n_lines] the records' windows (lo, hi) on their own: what tile_ranges_kernel scans (8 of a record's 48 bytes)
  DevBuf<int> maxhw;          // [maxhw | smally | n_items] = 2 * max_layers + 1 ints: one memset per prologue. [max_layers] max window half-width in grid points (+margin)
  int* smally = nullptr;      // inside maxhw: [max_layers] set when a line of that layer has a Weideman band with y < 1
  int* n_items = nullptr;     // inside maxhw: the counter of the hot-tile work list
  DevBuf<int2> ranges;        // [max_layers][max_tiles] candidate line range per line-sum tile
  DevBuf<LineRecSD> recsd;    // [max_layers][n_lines], allocated by the first speed-dependent prologue
  long long max_tiles = 0;
  DevBuf<double> env;         // device copy of T,p,qratio,weight,mass (packed)
  double scale = 0.0;
  // hot-tile split: work list and workspace sized from a HOST-side bound on the candidates per tile (no device read-back)
  DevBuf<SplitItem> items;    // the work list; its capacity is the bound it was sized for
  DevBuf<float> part_ws;      // [items.cap()][tile points]
  long long split_bound = 0;  // extra parts the current (grid, window) bound allows for; 0 = no tile can be hot
  double split_W = 0.0;       // window half-width [cm^-1] the bound was computed for (valid for any smaller one)
  double split_xmin = 0.0, split_step = 0.0;
  long long split_off = 0, split_n = 0;
  int split_layers = 0;
  const void* split_lines = nullptr;  // the table the bound was made for
  // explicit axis (rtx_line_prep_axis): device copy of the axis; `axis` tells which prologue ran last
  DevBuf<double> X;
  long long nx = 0;
  int axis = 0;
  DevBuf<double> twin;  // window temperatures of rtx_line_prep_window: device copy
  DevBuf<double> frac;  // diluent fractions of rtx_line_prep_mix / _axis_mix: device copy [n_dil][n_species][n_layers]
  // rtx_line_prep_dt: the derivative records [max_layers][n_lines], the device copy of dlnsw_h, and whether it ran last
  DevBuf<LineRecDT> drec;
  DevBuf<LineRecDT64> drec64;
  DevBuf<double> dlnsw;
  int dT = 0;
  // rtx_compute_tud_opts(RTX_CTUD_OD_SCRATCH): one byte per 64 points of the shard (= per row of a line-sum tile), padded to
  // whole tiles: written by the early TUD launch, read by the line-sum of the middle layers and the late TUD launch
  DevBuf<unsigned char> done;
};

// The layers of one line-sum launch (rtx_voigt_sum_layers): blockIdx.y < n_a -> layer k_a + y, else layer k_b + (y - n_a),
// n_y of them in all. done != nullptr: rows whose byte is set are neither needed nor stored, and a workgroup whose rows
// are all done returns before it loads a record. ranges: launch tile_ranges_kernel first (all layers; once per prologue).
struct VoigtLayers {
  int n_a, k_a, k_b, n_y;
  const unsigned char* done;
  bool ranges;
};
// rtx_voigt.hip: rtx_voigt_sum's fp32 sum restricted to `sel`; only where rtx_voigt_layers_ok(P) holds (the nodal kernel, no
// hot-tile parts, a grid prologue with lines)
__attribute__((visibility("hidden"))) bool rtx_voigt_layers_ok(const rtx_prep* P);
__attribute__((visibility("hidden"))) int rtx_voigt_sum_layers(const rtx_prep* P, const rtx_grid* grid, int n_layers, float* out_f32,
                                                                int64_t ld, void* stream, const VoigtLayers& sel);
