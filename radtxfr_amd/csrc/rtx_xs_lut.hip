// Optical depths from AFIT_XS cross-section tables: the table lives on the device as fp32 rows
// [row][x] (one row per molecule and (T, p) node, x fastest), and rtx_xs_od forms
//   OD[l][x] = sum_m sum_{c=0..3} w[l][m][c] * row[rows[l][m][c]][x]
// from host-made node rows and weights. One kernel, bandwidth-bound: no LDS, a handful of registers.
// rtx_xs_od_d forms the table's derivative columns, dOD/dT and dOD/dMF of each species asked for,
// from host-made derivative weights on the same rows, in one pass over the rows.
#include "rtx_common.h"

#define XS_BLOCK 256
#define XS_PER 4                       // points per thread: one 16-byte access
#define XS_TILE (XS_BLOCK * XS_PER)    // consecutive points owned by a workgroup

struct rtx_xs_lut {
  int n_mol;
  long long n_rows, nx, ldx;  // ldx: row stride in floats, a multiple of 4 (every row starts 16-byte aligned)
  DevBuf<float> data;         // [n_rows][ldx]
  int dev;
  // per-stream device copy of the terms of the last rtx_xs_od on that stream, rows then weights: two streams may run the
  // same table at once (compute_TUD_batch's two runners), and within a stream the copy is ordered behind the previous
  // kernel. It goes with the table (rtx_xs_lut_free: a call of the user's, not a static destructor).
  StreamScratch terms;
  // the same for rtx_xs_od_d, an array of its own: both entries can be live in one stream's call sequence
  StreamScratch terms_d;
};

// A workgroup owns XS_TILE consecutive points and walks all layers: a node's segment of the tile comes from HBM about
// once and from cache for every further layer (and corner) that names it. `rows` / `w` are wave-uniform: they travel
// through the scalar cache. Per point the sum is ONE fmaf chain in term order (molecule, then corner), terms with w == 0
// skipped and their row not read: a pure function of (table, layer, point), whatever the tile, x_off or n.
// VEC: x_off % 4 == 0 and the output rows are 16-byte aligned, so a thread's four points are one 16-byte load per term
// and one 16-byte store; the ragged end of the last tile, and every point otherwise, goes point by point.
template <bool VEC>
__global__ __launch_bounds__(XS_BLOCK) void xs_od_kernel(const float* __restrict__ tab, long long ldx, long long x_off, long long n,
                                                         int n_layers, int n_terms, const int* __restrict__ rows,
                                                         const float* __restrict__ w, float* __restrict__ od, long long ld) {
  const long long i0 = (long long)blockIdx.x * XS_TILE + (long long)threadIdx.x * XS_PER;
  if (i0 >= n) return;
  const float* __restrict__ src = tab + x_off + i0;
  const bool full = VEC && i0 + XS_PER <= n;
  for (int l = 0; l < n_layers; ++l) {
    const int* __restrict__ rl = rows + (size_t)l * n_terms;
    const float* __restrict__ wl = w + (size_t)l * n_terms;
    float* __restrict__ dst = od + (size_t)l * (size_t)ld + (size_t)i0;
    if (full) {
      float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      for (int t = 0; t < n_terms; ++t) {
        const float wt = wl[t];
        if (wt == 0.0f) continue;
        const float4 v = *reinterpret_cast<const float4*>(src + (size_t)rl[t] * (size_t)ldx);
        acc.x = fmaf(wt, v.x, acc.x);
        acc.y = fmaf(wt, v.y, acc.y);
        acc.z = fmaf(wt, v.z, acc.z);
        acc.w = fmaf(wt, v.w, acc.w);
      }
      *reinterpret_cast<float4*>(dst) = acc;
    } else {
      const int cnt = n - i0 < XS_PER ? (int)(n - i0) : XS_PER;
      for (int j = 0; j < cnt; ++j) {
        float acc = 0.0f;
        for (int t = 0; t < n_terms; ++t) {
          const float wt = wl[t];
          if (wt == 0.0f) continue;
          acc = fmaf(wt, src[(size_t)rl[t] * (size_t)ldx + j], acc);
        }
        dst[j] = acc;
      }
    }
  }
}

extern "C" int rtx_xs_tile_points(void) { return XS_TILE; }

extern "C" int rtx_xs_lut_create(int n_mol, int64_t n_rows, int64_t nx, rtx_xs_lut** out) {
  if (!out) RTX_FAIL("out is NULL");
  *out = nullptr;
  if (n_mol < 1 || n_rows < n_mol || nx < 1) RTX_FAIL("n_mol=%d n_rows=%lld nx=%lld", n_mol, (long long)n_rows, (long long)nx);
  if (n_rows > 0x7fffffffLL) RTX_FAIL("n_rows=%lld too large", (long long)n_rows);
  rtx_xs_lut* L = new rtx_xs_lut();
  L->n_mol = n_mol;
  L->n_rows = n_rows;
  L->nx = nx;
  L->ldx = (nx + 3) / 4 * 4;
  hipError_t e = hipGetDevice(&L->dev);
  const size_t bytes = (size_t)n_rows * (size_t)L->ldx * sizeof(float);
  if (e == hipSuccess && L->data.reserve((size_t)n_rows * (size_t)L->ldx)) e = hipErrorOutOfMemory;
  if (e == hipSuccess) e = hipMemset(L->data.get(), 0, bytes);  // the pad columns are read by no kernel; rows not yet set are 0
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    delete L;
    RTX_FAIL("rtx_xs_lut_create: %lld rows of %lld points (%.1f MB) -> %s", (long long)n_rows, (long long)nx, bytes / 1.0e6,
             hipGetErrorString(e));
  }
  *out = L;
  return 0;
}

extern "C" int rtx_xs_lut_free(rtx_xs_lut* L) {
  delete L;
  return 0;
}

extern "C" int64_t rtx_xs_lut_bytes(const rtx_xs_lut* L) {
  return L ? (int64_t)((size_t)L->n_rows * (size_t)L->ldx * sizeof(float)) : 0;
}

static int xs_check_rows(const rtx_xs_lut* L, int64_t row0, int64_t n_rows, const void* p) {
  if (!L || !p) RTX_FAIL("a required pointer is NULL");
  if (row0 < 0 || n_rows < 0 || row0 > L->n_rows - n_rows)
    RTX_FAIL("rows [%lld, %lld) outside the table's %lld", (long long)row0, (long long)(row0 + n_rows), (long long)L->n_rows);
  return 0;
}

extern "C" int rtx_xs_lut_set_rows(rtx_xs_lut* L, int64_t row0, int64_t n_rows, const float* rows_h, void* stream) {
  if (xs_check_rows(L, row0, n_rows, rows_h)) return 1;
  if (n_rows == 0) return 0;
  RTX_HIP(hipMemcpy2DAsync(L->data.get() + (size_t)row0 * (size_t)L->ldx, (size_t)L->ldx * sizeof(float), rows_h, (size_t)L->nx * sizeof(float),
                           (size_t)L->nx * sizeof(float), (size_t)n_rows, hipMemcpyHostToDevice, (hipStream_t)stream));
  return 0;
}

extern "C" int rtx_xs_lut_get_rows(const rtx_xs_lut* L, int64_t row0, int64_t n_rows, float* rows_h, void* stream) {
  if (xs_check_rows(L, row0, n_rows, rows_h)) return 1;
  if (n_rows == 0) return 0;
  RTX_HIP(hipMemcpy2DAsync(rows_h, (size_t)L->nx * sizeof(float), L->data.get() + (size_t)row0 * (size_t)L->ldx, (size_t)L->ldx * sizeof(float),
                           (size_t)L->nx * sizeof(float), (size_t)n_rows, hipMemcpyDeviceToHost, (hipStream_t)stream));
  RTX_HIP(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}

extern "C" int rtx_xs_od(rtx_xs_lut* L, int64_t x_offset, int64_t n, int n_layers, const int32_t* rows_h, const float* weight_h,
                         float* od_f32, int64_t ld, void* stream) {
  if (!L || !rows_h || !weight_h || !od_f32) RTX_FAIL("a required pointer is NULL");
  if (n_layers < 1) RTX_FAIL("n_layers=%d", n_layers);
  if (x_offset < 0 || n < 0 || x_offset > L->nx - n)
    RTX_FAIL("points [%lld, %lld) outside the table's axis of %lld points", (long long)x_offset, (long long)(x_offset + n),
             (long long)L->nx);
  if (ld < n) RTX_FAIL("ld=%lld smaller than n=%lld", (long long)ld, (long long)n);
  if (n == 0) return 0;
  if ((n + XS_TILE - 1) / XS_TILE > 0x7fffffffLL) RTX_FAIL("n=%lld too large", (long long)n);
  int dev = 0;
  RTX_HIP(hipGetDevice(&dev));
  if (dev != L->dev) RTX_FAIL("the table lives on device %d, the current device is %d", L->dev, dev);
  const int n_terms = 4 * L->n_mol;
  const size_t cnt = (size_t)n_layers * (size_t)n_terms;
  for (size_t t = 0; t < cnt; ++t) {  // a row index from outside is never trusted; a non-finite weight would poison a whole layer
    if (rows_h[t] < 0 || rows_h[t] >= L->n_rows) RTX_FAIL("rows_h[%zu]=%d outside the table's %lld rows", t, rows_h[t], (long long)L->n_rows);
    if (!isfinite(weight_h[t])) RTX_FAIL("weight_h[%zu] is not finite", t);
  }
  hipStream_t st = (hipStream_t)stream;
  void* base = nullptr;
  if (L->terms.get(st, cnt * (sizeof(int) + sizeof(float)), &base)) return 1;
  int* const rows_d = (int*)base;
  float* const w_d = (float*)(rows_d + cnt);
  RTX_HIP(hipMemcpyAsync(rows_d, rows_h, cnt * sizeof(int), hipMemcpyHostToDevice, st));  // pageable: staged before returning
  RTX_HIP(hipMemcpyAsync(w_d, weight_h, cnt * sizeof(float), hipMemcpyHostToDevice, st));
  const unsigned tiles = (unsigned)((n + XS_TILE - 1) / XS_TILE);
  const bool vec = (x_offset % 4 == 0) && (ld % 4 == 0) && (((uintptr_t)od_f32 & 15) == 0);
  if (vec)
    hipLaunchKernelGGL(xs_od_kernel<true>, dim3(tiles), dim3(XS_BLOCK), 0, st, L->data.get(), L->ldx, (long long)x_offset, (long long)n, n_layers,
                       n_terms, rows_d, w_d, od_f32, (long long)ld);
  else
    hipLaunchKernelGGL(xs_od_kernel<false>, dim3(tiles), dim3(XS_BLOCK), 0, st, L->data.get(), L->ldx, (long long)x_offset, (long long)n, n_layers,
                       n_terms, rows_d, w_d, od_f32, (long long)ld);
  RTX_LAUNCH_CHECK();
  return 0;
}

// ---- derivative columns -----------------------------------------------------------------------
#define XS_MAX_SPEC 16

// xs_od_kernel's frame (a workgroup owns XS_TILE points and walks all layers; rows, weights and slots are wave-uniform)
// with two weights per term: w_T for the temperature row and w_K for the row of the molecule's own K slot (slot[m] >= 0),
// 0 where the molecule has none. Per layer the molecules go in table order: a molecule's (up to four) corner rows are
// loaded once, together, a row whose two weights are both 0 not at all; then the temperature chain takes the terms with
// w_T != 0, and a molecule with a slot forms and stores that slot's value from the terms with w_K != 0 -- distinct slots
// are distinct molecules, so one value is live besides the temperature chain. Every output value is ONE fmaf chain from 0
// in term order over the terms whose weight for that output is not 0: what xs_od_kernel gives for those weights, bit for
// bit, and a pure function of (table, layer, point). dT / K may be NULL (then w_T is all 0 / every slot is -1).
template <bool VEC>
__global__ __launch_bounds__(XS_BLOCK) void xs_od_d_kernel(const float* __restrict__ tab, long long ldx, long long x_off, long long n,
                                                           int n_layers, int n_mol, const int* __restrict__ rows,
                                                           const float* __restrict__ w_T, const float* __restrict__ w_K,
                                                           const int* __restrict__ slot, float* __restrict__ dT, float* __restrict__ K,
                                                           long long ld) {
  const long long i0 = (long long)blockIdx.x * XS_TILE + (long long)threadIdx.x * XS_PER;
  if (i0 >= n) return;
  const float* __restrict__ src = tab + x_off + i0;
  const int cnt = n - i0 < XS_PER ? (int)(n - i0) : XS_PER;
  const bool full = VEC && cnt == XS_PER;
  for (int l = 0; l < n_layers; ++l) {
    float accT[XS_PER] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int m = 0; m < n_mol; ++m) {
      const size_t t0 = ((size_t)l * (size_t)n_mol + (size_t)m) * 4;
      const int sl = slot[m];
      float wt[4], wk[4], v[4][XS_PER];
#pragma unroll
      for (int c = 0; c < 4; ++c) {  // the loads of the molecule's rows, issued together
        wt[c] = w_T[t0 + c];
        wk[c] = w_K[t0 + c];
#pragma unroll
        for (int j = 0; j < XS_PER; ++j) v[c][j] = 0.0f;
        if (wt[c] != 0.0f || wk[c] != 0.0f) {
          const float* __restrict__ p = src + (size_t)rows[t0 + c] * (size_t)ldx;
          if (full) {
            const float4 q = *reinterpret_cast<const float4*>(p);
            v[c][0] = q.x;
            v[c][1] = q.y;
            v[c][2] = q.z;
            v[c][3] = q.w;
          } else {
#pragma unroll
            for (int j = 0; j < XS_PER; ++j)
              if (j < cnt) v[c][j] = p[j];
          }
        }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (wt[c] != 0.0f) {
#pragma unroll
          for (int j = 0; j < XS_PER; ++j) accT[j] = fmaf(wt[c], v[c][j], accT[j]);
        }
      if (sl >= 0) {
        float a[XS_PER] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (wk[c] != 0.0f) {
#pragma unroll
            for (int j = 0; j < XS_PER; ++j) a[j] = fmaf(wk[c], v[c][j], a[j]);
          }
        float* __restrict__ dst = K + ((size_t)sl * (size_t)n_layers + (size_t)l) * (size_t)ld + (size_t)i0;
        if (full) {
          *reinterpret_cast<float4*>(dst) = make_float4(a[0], a[1], a[2], a[3]);
        } else {
#pragma unroll
          for (int j = 0; j < XS_PER; ++j)
            if (j < cnt) dst[j] = a[j];
        }
      }
    }
    if (dT) {
      float* __restrict__ dst = dT + (size_t)l * (size_t)ld + (size_t)i0;
      if (full) {
        *reinterpret_cast<float4*>(dst) = make_float4(accT[0], accT[1], accT[2], accT[3]);
      } else {
#pragma unroll
        for (int j = 0; j < XS_PER; ++j)
          if (j < cnt) dst[j] = accT[j];
      }
    }
  }
}

extern "C" int rtx_xs_od_d(rtx_xs_lut* L, int64_t x_offset, int64_t n, int n_layers, const int32_t* rows_h, const float* weight_dT_h,
                           int n_spec, const int32_t* spec_mol_h, const float* weight_K_h, float* dOD_dT, float* K, int64_t ld,
                           void* stream, unsigned flags) {
  if (!L || !rows_h) RTX_FAIL("a required pointer is NULL");
  if (flags != 0) RTX_FAIL("rtx_xs_od_d: flags=%u, none is defined", flags);
  if (!dOD_dT && !K) RTX_FAIL("rtx_xs_od_d: dOD_dT and K are both NULL");
  if (n_layers < 1) RTX_FAIL("n_layers=%d", n_layers);
  if (n_spec < 0 || n_spec > XS_MAX_SPEC) RTX_FAIL("rtx_xs_od_d: n_spec=%d, supported 0..%d", n_spec, XS_MAX_SPEC);
  if (dOD_dT && !weight_dT_h) RTX_FAIL("rtx_xs_od_d: dOD_dT needs weight_dT_h");
  if (n_spec > 0 && !K) RTX_FAIL("rtx_xs_od_d: K is NULL but n_spec=%d", n_spec);
  if (n_spec > 0 && (!spec_mol_h || !weight_K_h)) RTX_FAIL("rtx_xs_od_d: K needs spec_mol_h and weight_K_h");
  if (x_offset < 0 || n < 0 || x_offset > L->nx - n)
    RTX_FAIL("points [%lld, %lld) outside the table's axis of %lld points", (long long)x_offset, (long long)(x_offset + n),
             (long long)L->nx);
  if (ld < n) RTX_FAIL("ld=%lld smaller than n=%lld", (long long)ld, (long long)n);
  const int n_mol = L->n_mol;
  const size_t cnt = (size_t)n_layers * (size_t)n_mol * 4;
  // one host block, staged in one copy: rows | w_T | w_K (a molecule's slot weights at its own terms, 0 elsewhere) | slot
  std::vector<int32_t> head(3 * cnt + (size_t)n_mol);  // zero-filled; floats are written through float pointers below
  int32_t* const rows_s = head.data();
  float* const wT_s = (float*)(head.data() + cnt);
  float* const wK_s = (float*)(head.data() + 2 * cnt);
  int32_t* const slot_s = head.data() + 3 * cnt;
  for (int m = 0; m < n_mol; ++m) slot_s[m] = -1;
  for (int s = 0; s < n_spec; ++s) {
    const int m = spec_mol_h[s];
    if (m < 0 || m >= n_mol) RTX_FAIL("spec_mol_h[%d]=%d outside the table's %d molecules", s, m, n_mol);
    if (slot_s[m] >= 0) RTX_FAIL("spec_mol_h[%d]=%d names a molecule twice: the species must be distinct", s, m);
    slot_s[m] = s;
  }
  for (size_t t = 0; t < cnt; ++t) {  // a row index from outside is never trusted; a non-finite weight would poison a whole layer
    if (rows_h[t] < 0 || rows_h[t] >= L->n_rows) RTX_FAIL("rows_h[%zu]=%d outside the table's %lld rows", t, rows_h[t], (long long)L->n_rows);
    rows_s[t] = rows_h[t];
    if (dOD_dT) {
      if (!isfinite(weight_dT_h[t])) RTX_FAIL("weight_dT_h[%zu] is not finite", t);
      wT_s[t] = weight_dT_h[t];
    }
  }
  for (int s = 0; s < n_spec; ++s)
    for (int l = 0; l < n_layers; ++l)
      for (int c = 0; c < 4; ++c) {
        const size_t t = ((size_t)s * (size_t)n_layers + (size_t)l) * 4 + (size_t)c;
        if (!isfinite(weight_K_h[t])) RTX_FAIL("weight_K_h[%zu] is not finite", t);
        wK_s[((size_t)l * (size_t)n_mol + (size_t)spec_mol_h[s]) * 4 + (size_t)c] = weight_K_h[t];
      }
  if (n == 0 || (!dOD_dT && n_spec == 0)) return 0;
  if ((n + XS_TILE - 1) / XS_TILE > 0x7fffffffLL) RTX_FAIL("n=%lld too large", (long long)n);
  int dev = 0;
  RTX_HIP(hipGetDevice(&dev));
  if (dev != L->dev) RTX_FAIL("the table lives on device %d, the current device is %d", L->dev, dev);
  hipStream_t st = (hipStream_t)stream;
  void* base = nullptr;
  if (L->terms_d.get(st, head.size() * sizeof(int32_t), &base)) return 1;
  RTX_HIP(hipMemcpyAsync(base, head.data(), head.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));  // pageable: staged before returning
  const int* const rows_d = (const int*)base;
  const float* const wT_d = (const float*)(rows_d + cnt);
  const float* const wK_d = wT_d + cnt;
  const int* const slot_d = rows_d + 3 * cnt;
  float* const K_used = n_spec > 0 ? K : nullptr;
  const unsigned tiles = (unsigned)((n + XS_TILE - 1) / XS_TILE);
  const bool vec = (x_offset % 4 == 0) && (ld % 4 == 0) && (((uintptr_t)dOD_dT & 15) == 0) && (((uintptr_t)K_used & 15) == 0);
  if (vec)
    hipLaunchKernelGGL(xs_od_d_kernel<true>, dim3(tiles), dim3(XS_BLOCK), 0, st, L->data.get(), L->ldx, (long long)x_offset, (long long)n,
                       n_layers, n_mol, rows_d, wT_d, wK_d, slot_d, dOD_dT, K_used, (long long)ld);
  else
    hipLaunchKernelGGL(xs_od_d_kernel<false>, dim3(tiles), dim3(XS_BLOCK), 0, st, L->data.get(), L->ldx, (long long)x_offset, (long long)n,
                       n_layers, n_mol, rows_d, wT_d, wK_d, slot_d, dOD_dT, K_used, (long long)ld);
  RTX_LAUNCH_CHECK();
  return 0;
}
