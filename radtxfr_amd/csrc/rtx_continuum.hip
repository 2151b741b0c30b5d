// Tabulated continuum absorption added to a block of optical depths: per component c a uniform
// node axis (v0, dv, n) and per layer a host-made fp32 row A[c][l][n] (column amount, density scaling and the
// self / foreign coefficients folded in, radtxfr_amd/continuum.py: layer_tables), and
//   od[l][i] += R(nu_i, T_l) * sum_c max(0, sum_{k<4} L_k(t) * A[c][l][j0 + k]),   R = nu tanh(c2 nu / (2 T))
// with the four-node Lagrange cubic of the definition. One kernel, bandwidth-bound: it reads and writes the block once per
// CT_GROUP components; no LDS.
#include "rtx_continuum_common.h"

// Scratch of rtx_continuum_add per (device, stream): [ContComp x n_comp][float c2/T x n_layers][tables]. Made with `new`,
// never destroyed (rtx_devmem.h).
static StreamScratch* const g_cont_scratch = new StreamScratch();

// A workgroup owns CT_TILE consecutive points and walks all layers. Per point and component the stencil start j0 and the
// four Lagrange weights are made once, from the fp64 wavenumber of the GLOBAL point index (nu - nu_j0 is formed in fp64,
// then rounded), and reused for every layer; a point outside the component's axis gets weights 0. c2/T_l and the row
// addresses are wave-uniform. Where a whole wave sits on one stencil (the usual case: grid step << node spacing) the four
// node values of a (layer, component) are read once for the wave through a uniform address, else lane by lane; both forms
// run the same fp32 operations on the same values, so a point's result is a pure function of (tables, layer, global
// index), whatever the tile, offset or n.
// VEC: ld % 4 == 0 and the rows are 16-byte aligned: a thread's four points are one 16-byte load and one 16-byte store,
// the next layer's load issued before this layer's store; the ragged end, and every point otherwise, goes point by point.
template <bool VEC>
__global__ __launch_bounds__(CT_BLOCK) void continuum_add_kernel(GridDev g, int n_layers, int n_comp, const ContComp* __restrict__ comps,
                                                                 const float* __restrict__ c2T, const float* __restrict__ tab,
                                                                 long long ld_nodes, float* od, long long ld) {
  const long long i0 = (long long)blockIdx.x * CT_TILE + (long long)threadIdx.x * CT_PER;
  if (i0 >= g.n) return;
  const int cnt = g.n - i0 < CT_PER ? (int)(g.n - i0) : CT_PER;
  const bool full = VEC && cnt == CT_PER;
  double nu[CT_PER];
  float nuf[CT_PER];
#pragma unroll
  for (int j = 0; j < CT_PER; ++j) {
    nu[j] = grid_x(g, g.offset + i0 + (j < cnt ? j : cnt - 1));  // a point past the end repeats the last one; it is never stored
    nuf[j] = (float)nu[j];
  }
  for (int c0 = 0; c0 < n_comp; c0 += CT_GROUP) {
    const int nc = n_comp - c0 < CT_GROUP ? n_comp - c0 : CT_GROUP;
    int j0[CT_GROUP][CT_PER];
    float L[CT_GROUP][CT_PER][4];
    int jf[CT_GROUP];
    bool uni[CT_GROUP];
#pragma unroll
    for (int c = 0; c < CT_GROUP; ++c) {
      jf[c] = 0;
      uni[c] = true;
      if (c < nc) {
        const ContComp cc = comps[c0 + c];
        bool same = true;
#pragma unroll
        for (int j = 0; j < CT_PER; ++j) j0[c][j] = cont_stencil(cc, nu[j], L[c][j]);
        jf[c] = __builtin_amdgcn_readfirstlane(j0[c][0]);
#pragma unroll
        for (int j = 0; j < CT_PER; ++j) same = same && j0[c][j] == jf[c];
        uni[c] = __all(same) != 0;
      }
    }
    float4 cur = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (full) cur = *reinterpret_cast<const float4*>(od + (size_t)i0);
    for (int l = 0; l < n_layers; ++l) {
      float* dst = od + (size_t)l * (size_t)ld + (size_t)i0;
      float4 nxt = cur;
      if (full && l + 1 < n_layers) nxt = *reinterpret_cast<const float4*>(dst + (size_t)ld);
      const float k = c2T[l];
      float acc[CT_PER] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int c = 0; c < CT_GROUP; ++c) {
        if (c < nc) {
          const float* __restrict__ row = tab + ((size_t)(c0 + c) * (size_t)n_layers + (size_t)l) * (size_t)ld_nodes;
          if (uni[c]) {
            const float a0 = row[jf[c]], a1 = row[jf[c] + 1], a2 = row[jf[c] + 2], a3 = row[jf[c] + 3];
#pragma unroll
            for (int j = 0; j < CT_PER; ++j) {
              const float s = cont_stencil_sum(L[c][j], a0, a1, a2, a3);
              acc[j] += fmaxf(s, 0.0f);
            }
          } else {
#pragma unroll
            for (int j = 0; j < CT_PER; ++j) {
              const float* __restrict__ a = row + j0[c][j];
              const float s = cont_stencil_sum(L[c][j], a[0], a[1], a[2], a[3]);
              acc[j] += fmaxf(s, 0.0f);
            }
          }
        }
      }
      float add[CT_PER];
#pragma unroll
      for (int j = 0; j < CT_PER; ++j) add[j] = radiation_term(nuf[j], nuf[j] * k) * acc[j];
      if (full) {
        cur.x += add[0];
        cur.y += add[1];
        cur.z += add[2];
        cur.w += add[3];
        *reinterpret_cast<float4*>(dst) = cur;
        cur = nxt;
      } else {
        for (int j = 0; j < cnt; ++j) dst[j] += add[j];
      }
    }
  }
}

extern "C" int rtx_continuum_tile_points(void) { return CT_TILE; }

extern "C" int rtx_continuum_add(const rtx_grid* grid, int n_layers, const double* T_h, int n_comp, const double* v0_h,
                                 const double* dv_h, const int32_t* n_nodes_h, const float* tables_h, int64_t ld_nodes, float* od_f32,
                                 int64_t ld, void* stream, unsigned flags) {
  if (!grid || !T_h || !v0_h || !dv_h || !n_nodes_h || !tables_h || !od_f32) RTX_FAIL("a required pointer is NULL");
  if (flags != 0) RTX_FAIL("rtx_continuum_add: flags=%u, none is defined", flags);
  if (rtx_check_grid(grid)) return 1;
  if (n_layers < 1 || n_comp < 1) RTX_FAIL("n_layers=%d n_comp=%d", n_layers, n_comp);
  if (ld < grid->n) RTX_FAIL("ld=%lld smaller than n=%lld", (long long)ld, (long long)grid->n);
  if (ld_nodes < 4 || ld_nodes > 0x7fffffffLL) RTX_FAIL("ld_nodes=%lld", (long long)ld_nodes);
  std::vector<char> head((size_t)n_comp * sizeof(ContComp) + (size_t)n_layers * sizeof(float));
  ContComp* const comps = (ContComp*)head.data();
  float* const c2T = (float*)(comps + n_comp);
  for (int c = 0; c < n_comp; ++c) {
    const int nn = n_nodes_h[c];
    if (nn < 4 || nn > ld_nodes) RTX_FAIL("component %d: %d nodes (at least 4, at most ld_nodes=%lld)", c, nn, (long long)ld_nodes);
    if (!isfinite(v0_h[c]) || !isfinite(dv_h[c]) || !(dv_h[c] > 0.0)) RTX_FAIL("component %d: v0=%g dv=%g", c, v0_h[c], dv_h[c]);
    comps[c].v0 = v0_h[c];
    comps[c].dv = dv_h[c];
    comps[c].vend = v0_h[c] + (double)(nn - 1) * dv_h[c];
    comps[c].n = nn;
    comps[c].pad = 0;
    for (int l = 0; l < n_layers; ++l) {  // a non-finite node value would poison every point of its stencils
      const float* const row = tables_h + ((size_t)c * (size_t)n_layers + (size_t)l) * (size_t)ld_nodes;
      for (int j = 0; j < nn; ++j)
        if (!isfinite(row[j])) RTX_FAIL("tables_h[%d][%d][%d] is not finite", c, l, j);
    }
  }
  for (int l = 0; l < n_layers; ++l) {
    if (!isfinite(T_h[l]) || !(T_h[l] > 0.0)) RTX_FAIL("T_h[%d]=%g", l, T_h[l]);
    c2T[l] = (float)(CT_C2 / T_h[l]);
  }
  if (grid->n == 0) return 0;
  if ((grid->n + CT_TILE - 1) / CT_TILE > 0x7fffffffLL) RTX_FAIL("n=%lld too large", (long long)grid->n);
  hipStream_t st = (hipStream_t)stream;
  const size_t head_bytes = (head.size() + 15) / 16 * 16;
  const size_t tab_bytes = (size_t)n_comp * (size_t)n_layers * (size_t)ld_nodes * sizeof(float);
  void* base = nullptr;
  if (g_cont_scratch->get(stream, head_bytes + tab_bytes, &base)) return 1;
  float* const tab_d = (float*)((char*)base + head_bytes);
  RTX_HIP(hipMemcpyAsync(base, head.data(), head.size(), hipMemcpyHostToDevice, st));  // pageable: staged before returning
  RTX_HIP(hipMemcpyAsync(tab_d, tables_h, tab_bytes, hipMemcpyHostToDevice, st));
  const ContComp* const comps_d = (const ContComp*)base;
  const float* const c2T_d = (const float*)(comps_d + n_comp);
  const unsigned tiles = (unsigned)((grid->n + CT_TILE - 1) / CT_TILE);
  const bool vec = (ld % 4 == 0) && (((uintptr_t)od_f32 & 15) == 0);
  if (vec)
    hipLaunchKernelGGL(continuum_add_kernel<true>, dim3(tiles), dim3(CT_BLOCK), 0, st, to_dev(grid), n_layers, n_comp, comps_d, c2T_d, tab_d,
                       (long long)ld_nodes, od_f32, (long long)ld);
  else
    hipLaunchKernelGGL(continuum_add_kernel<false>, dim3(tiles), dim3(CT_BLOCK), 0, st, to_dev(grid), n_layers, n_comp, comps_d, c2T_d, tab_d,
                       (long long)ld_nodes, od_f32, (long long)ld);
  RTX_LAUNCH_CHECK();
  return 0;
}
