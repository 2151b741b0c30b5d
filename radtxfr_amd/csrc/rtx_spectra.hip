// hapi's spectrum functions (transmittanceSpectrum / absorptionSpectrum / radianceSpectrum, misc/hapi.py:11582-11680) and
// the convolution behind convolveSpectrum* (misc/hapi.py:11826-11900: numpy.convolve with a slit function of 1e2-1e5
// points). Two kernels, fp64 like the reference: one elementwise, one dense FIR.
#include <string.h>

#include <mutex>
#include <vector>

#include "rtx_common.h"

// hapi's own constants (misc/hapi.py:84-86), not radiative_transfer.py's c1 / c2
#define HAPI_CBOLTS 1.380648813e-16
#define HAPI_CC 2.99792458e10
#define HAPI_HH 6.626196e-27

// out[r][i] = exp(-k l) | 1 - exp(-k l) | (1 - exp(-k l)) * a nu^3 / (exp(hc nu / kT) - 1) * 1e-7, in the reference's
// order of operations (the translation unit is compiled with -ffp-contract=off).
template <typename T>
__global__ __launch_bounds__(256) void hapi_spectrum_kernel(int kind, GridDev g, const double* __restrict__ X, const T* __restrict__ k,
                                                            long long n, long long ld, double l, double a, double hc, double kT,
                                                            double* __restrict__ out, long long ld_out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t row = blockIdx.y;
  const double e = exp(-((double)k[row * (size_t)ld + (size_t)i] * l));
  double v = e;
  if (kind != RTX_SPECTRUM_TRANSMITTANCE) v = 1.0 - e;
  if (kind == RTX_SPECTRUM_RADIANCE) {
    const double nu = X ? X[i] : grid_x(g, g.offset + i);
    v = v * (a * (nu * nu * nu) / (exp(hc * nu / kT) - 1.0) * 1.0e-7);
  }
  out[row * (size_t)ld_out + (size_t)i] = v;
}

extern "C" int rtx_hapi_spectrum(int kind, const rtx_grid* grid, const double* X, const void* k, int k_is_f64, int n_rows, int64_t n,
                                 int64_t ld, double l, double T, double* out, int64_t ld_out, void* stream) {
  if (!k || !out) RTX_FAIL("a required pointer is NULL");
  if (kind < RTX_SPECTRUM_TRANSMITTANCE || kind > RTX_SPECTRUM_RADIANCE) RTX_FAIL("kind=%d", kind);
  if (n_rows < 1 || n_rows > 65535) RTX_FAIL("n_rows=%d outside [1,65535]", n_rows);
  if (n < 0 || ld < n || ld_out < n) RTX_FAIL("n=%lld ld=%lld ld_out=%lld", (long long)n, (long long)ld, (long long)ld_out);
  if (n == 0) return 0;
  GridDev g = {};
  if (kind == RTX_SPECTRUM_RADIANCE && !X) {
    if (!grid) RTX_FAIL("radiance needs the wavenumbers: X or grid");
    if (rtx_check_grid(grid)) return 1;
    if (grid->n != n) RTX_FAIL("grid.n=%lld but n=%lld", (long long)grid->n, (long long)n);
    g = to_dev(grid);
  }
  const double a = 2.0 * HAPI_HH * (HAPI_CC * HAPI_CC), hc = HAPI_HH * HAPI_CC, kT = HAPI_CBOLTS * T;
  const dim3 blocks((unsigned)((n + 255) / 256), (unsigned)n_rows);
  if (k_is_f64)
    hipLaunchKernelGGL(hapi_spectrum_kernel<double>, blocks, dim3(256), 0, (hipStream_t)stream, kind, g, X, (const double*)k, (long long)n,
                       (long long)ld, l, a, hc, kT, out, (long long)ld_out);
  else
    hipLaunchKernelGGL(hapi_spectrum_kernel<float>, blocks, dim3(256), 0, (hipStream_t)stream, kind, g, X, (const float*)k, (long long)n,
                       (long long)ld, l, a, hc, kT, out, (long long)ld_out);
  RTX_LAUNCH_CHECK();
  return 0;
}

// ---- dense FIR: a window of the zero-padded linear convolution -------------------------------------------------------
// out[r][o] = out_scale * sum_{k=0}^{m-1} taps[k] * in[r][first + o - k]   (samples outside [0,n) are 0),  o in [0,n_out).
// A workgroup owns FS_TILE consecutive outputs of one row and walks the taps in chunks of FS_CHUNK: the chunk's input span
// is staged in LDS (converted to fp64, zero outside the row), each thread keeps FS_PER = 8 running sums of 8 CONSECUTIVE
// outputs, and per group of 8 taps reads the 15 samples the 8 x 8 (output, tap) pairs touch once into registers: 15 LDS
// reads feed 64 fp64 FMAs. The taps are wave-uniform, so they come through the scalar cache into SGPRs and are the FMA's
// scalar operand: no LDS traffic for them. A thread's outputs are 8 samples apart from its neighbour's, so the span is stored
// with two pad words per 8 samples: lane stride 10 doubles = 80 bytes, so a thread's samples are 16-byte aligned
// (ds_read_b128, the full LDS rate) and the 16 lanes of each ds_read_b128 group start on 16 distinct four-bank slots.
// Every output is one fma chain over k = 0 .. m-1 in ascending order, whatever the tile, the chunk or the row count:
// bit-identical run to run and independent of n_rows.
#define FS_BLOCK 256
#define FS_PER 8
#define FS_TILE (FS_BLOCK * FS_PER)
#define FS_CHUNK 1024
#define FS_SPAN (FS_TILE + FS_CHUNK)  // samples staged per chunk (FS_TILE + FS_CHUNK - 1 are read)
#define FS_LDS (FS_SPAN / 8 * 10)     // LDS = 30 KiB
static_assert(FS_PER == 8 && FS_CHUNK % 8 == 0, "the padded layout below is written for groups of 8");

template <typename T>
__global__ __launch_bounds__(FS_BLOCK) void fir_same_kernel(const T* __restrict__ in, long long ld_in, long long n,
                                                            const double* __restrict__ taps, long long m, double out_scale,
                                                            long long first, long long n_out, double* __restrict__ out,
                                                            long long ld_out) {
  __shared__ __attribute__((aligned(16))) double s_x[FS_LDS];
  const size_t row = blockIdx.y;
  const long long o0 = (long long)blockIdx.x * FS_TILE;
  const T* __restrict__ src = in + row * (size_t)ld_in;
  const int t = threadIdx.x;
  double acc[FS_PER];
#pragma unroll
  for (int j = 0; j < FS_PER; ++j) acc[j] = 0.0;
  for (long long k0 = 0; k0 < m; k0 += FS_CHUNK) {
    const int kc = m - k0 < FS_CHUNK ? (int)(m - k0) : FS_CHUNK;
    const double* __restrict__ tp = taps + k0;
    // staged sample s = in[base + s]; output o of the tile and local tap kl meet at s = FS_CHUNK - 1 + o - kl
    const long long base = first + o0 - k0 - (FS_CHUNK - 1);
    __syncthreads();
    for (int s = t; s < FS_SPAN; s += FS_BLOCK) {
      const long long idx = base + s;
      s_x[s + 2 * (s >> 3)] = (idx >= 0 && idx < n) ? (double)src[idx] : 0.0;
    }
    __syncthreads();
    int kl = 0;
    for (; kl + 8 <= kc; kl += 8) {
      // s = (FS_CHUNK - 8 - kl) + 8 t + e,  e = 7 + j - u in [0, 14]: eight-sample block (FS_CHUNK - 8 - kl) / 8 + t, offset e
      const double* __restrict__ p = s_x + 10 * (((FS_CHUNK - 8 - kl) >> 3) + t);
      double w[15], tk[8];
#pragma unroll
      for (int e = 0; e < 15; ++e) w[e] = p[e + 2 * (e >> 3)];
#pragma unroll
      for (int u = 0; u < 8; ++u) tk[u] = tp[kl + u];
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int j = 0; j < FS_PER; ++j) acc[j] = fma(tk[u], w[7 + j - u], acc[j]);
    }
    for (; kl < kc; ++kl) {  // the last m % 8 taps
      const double tk = tp[kl];
#pragma unroll
      for (int j = 0; j < FS_PER; ++j) {
        const int c = FS_CHUNK - 1 - kl + j;
        acc[j] = fma(tk, s_x[10 * t + c + 2 * (c >> 3)], acc[j]);
      }
    }
  }
  const long long o = o0 + (long long)t * FS_PER;
#pragma unroll
  for (int j = 0; j < FS_PER; ++j)
    if (o + j < n_out) out[row * (size_t)ld_out + (size_t)(o + j)] = acc[j] * out_scale;
}

extern "C" int rtx_fir_tile_points(void) { return FS_TILE; }
extern "C" int rtx_fir_chunk_taps(void) { return FS_CHUNK; }

extern "C" int rtx_fir_same(const void* in, int in_is_f64, int64_t ld_in, int n_rows, int64_t n, const double* taps_h, int64_t m,
                            double out_scale, int64_t first, int64_t n_out, double* out, int64_t ld_out, void* stream) {
  if (!in || !taps_h || !out) RTX_FAIL("a required pointer is NULL");
  if (m < 1) RTX_FAIL("m=%lld: the filter needs at least one tap", (long long)m);
  if (n < 1) RTX_FAIL("n=%lld: the rows need at least one sample", (long long)n);
  if (n_rows < 1) RTX_FAIL("n_rows=%d", n_rows);
  if (first < 0 || n_out < 0 || first > n + m - 1 - n_out)
    RTX_FAIL("window [%lld, %lld) lies outside the %lld points of the full convolution", (long long)first, (long long)(first + n_out),
             (long long)(n + m - 1));
  if (ld_in < n || ld_out < n_out) RTX_FAIL("leading dimension smaller than the row");
  if (n_out == 0) return 0;
  if ((n_out + FS_TILE - 1) / FS_TILE > 0x7fffffffLL) RTX_FAIL("n_out=%lld too large", (long long)n_out);
  hipStream_t st = (hipStream_t)stream;
  // device copies of the slits seen so far: a hit costs a memcmp, only a new slit is uploaded
  static DevTableCache<double>* const cache = new DevTableCache<double>(16);
  int dev = 0;
  RTX_HIP(hipGetDevice(&dev));
  DevTableCache<double>::Hit taps;  // holds the cache's lock until this function returns, after the launches
  if (cache->get(dev, taps_h, (size_t)m * sizeof(double), [&](std::vector<double>& h) { h.assign(taps_h, taps_h + m); return 0; }, &taps))
    return 1;
  const double* d_taps = taps.d;
  const unsigned tiles = (unsigned)((n_out + FS_TILE - 1) / FS_TILE);
  for (int r0 = 0; r0 < n_rows; r0 += 65535) {  // grid.y holds 65535 rows
    const int nr = n_rows - r0 < 65535 ? n_rows - r0 : 65535;
    const dim3 blocks(tiles, (unsigned)nr);
    const size_t esz = in_is_f64 ? sizeof(double) : sizeof(float);
    const void* src = (const char*)in + (size_t)r0 * (size_t)ld_in * esz;
    double* dst = out + (size_t)r0 * (size_t)ld_out;
    if (in_is_f64)
      hipLaunchKernelGGL(fir_same_kernel<double>, blocks, dim3(FS_BLOCK), 0, st, (const double*)src, (long long)ld_in, (long long)n, d_taps,
                         (long long)m, out_scale, (long long)first, (long long)n_out, dst, (long long)ld_out);
    else
      hipLaunchKernelGGL(fir_same_kernel<float>, blocks, dim3(FS_BLOCK), 0, st, (const float*)src, (long long)ld_in, (long long)n, d_taps,
                         (long long)m, out_scale, (long long)first, (long long)n_out, dst, (long long)ld_out);
    RTX_LAUNCH_CHECK();
  }
  return 0;
}
