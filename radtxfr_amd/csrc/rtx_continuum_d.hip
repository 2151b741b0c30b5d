// Derivatives of the tabulated continuum added to the columns the TUD derivative entries take:
// with s_c = sum_{k<4} L_k(t) A[c][l][j0 + k] the stencil sum rtx_continuum_add clamps, m_c = [s_c > 0], s_T and s_x the
// same stencil and weights on the host-made rows dA/dT and dA/dMF (radtxfr_amd/continuum.py: layer_tables_d),
//   dOD_dT[l][i]     += R_T sum_c max(0, s_c) + R sum_c m_c s_T,c       R = nu tanh(c2 nu / (2 T)), R_T = dR/dT
//   K[slot][l][i]    += R sum_{c: slot_c = slot} m_c s_x,c
// One kernel, bandwidth-bound: per CT_GROUP components it reads and writes each destination row once; no LDS.
#include "rtx_continuum_common.h"

// Scratch of rtx_continuum_add_d per (device, stream):
// [ContComp x n_comp][ContJob x CT_JOBS per group][float c2/T x n_layers][float 1/T x n_layers][tables A, dA/dT, dA/dMF].
// Made with `new`, never destroyed (rtx_devmem.h).
static StreamScratch* const g_cont_d_scratch = new StreamScratch();

// R as radiation_term forms it (the same operations) and R_T = -nu (x / (2T)) sech^2(x/2), x = c2 nu / T, from the one
// exponential: sech^2(x/2) = 4 e / (1 + e)^2; below the series threshold 1 - tanh^2 with the series' tanh (no cancellation:
// tanh <= 1/16 there).
__device__ __forceinline__ void radiation_terms_d(float nu, float x, float invT, float& R, float& R_T) {
  float th, sech2;
  if (x < 0.125f) {
    th = tanh_half_series(x);
    sech2 = fmaf(-th, th, 1.0f);
  } else {
    const float e = __builtin_amdgcn_exp2f(-x * (float)LOG2E);
    const float r = __builtin_amdgcn_rcpf(1.0f + e);
    th = (1.0f - e) * r;
    sech2 = (4.0f * e) * (r * r);
  }
  R = nu * th;
  R_T = -nu * ((0.5f * x) * invT) * sech2;
}

// The stencil sums of a thread's points on one table row: through a wave-uniform address where the whole wave sits on one
// stencil, else lane by lane; the same arithmetic on the same values either way.
__device__ __forceinline__ void cont_sums(const float* __restrict__ row, bool uni, int jf, const int (&j0)[CT_PER],
                                          const float (&L)[CT_PER][4], float (&s)[CT_PER]) {
  if (uni) {
    const float a0 = row[jf], a1 = row[jf + 1], a2 = row[jf + 2], a3 = row[jf + 3];
#pragma unroll
    for (int j = 0; j < CT_PER; ++j) s[j] = cont_stencil_sum(L[j], a0, a1, a2, a3);
  } else {
#pragma unroll
    for (int j = 0; j < CT_PER; ++j) {
      const float* __restrict__ a = row + j0[j];
      s[j] = cont_stencil_sum(L[j], a[0], a[1], a[2], a[3]);
    }
  }
}

// One destination row of a group of components: dOD_dT's (slot -1) or K's row of `slot`, and the bits of the group's
// components that add to it. The host lists them per group, a mask of 0 ending the list (CT_JOBS entries per group: the
// temperature row, at most CT_GROUP slots, the end).
#define CT_JOBS (CT_GROUP + 2)
struct ContJob {
  int slot, mask;
};

// Stencils and weights per point and component exactly as continuum_add_kernel makes them (rtx_continuum_common.h), so
// m_c = [s_c > 0] is set where that kernel added something. Per layer R and R_T cost one exponential per point. Each
// destination row of a group's job list is read and written once per group: the contributions of the job's components
// are summed first, then added to the block, so on a block of zeros the result is the derivative itself. A point's result
// is a pure function of (tables, layer, global index).
// VEC: ld % 4 == 0 and both blocks 16-byte aligned: a thread's four points are one 16-byte load and one 16-byte store; the
// ragged end, and every point otherwise, goes point by point.
template <bool VEC>
__global__ __launch_bounds__(CT_BLOCK) void continuum_add_d_kernel(GridDev g, int n_layers, int n_comp, const ContComp* __restrict__ comps,
                                                                   const ContJob* __restrict__ jobs, const float* __restrict__ c2T,
                                                                   const float* __restrict__ invT, const float* __restrict__ tab,
                                                                   int tab_stride, int ld_nodes, float* dT, float* K, long long ld) {
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
  for (int c0 = 0; c0 < n_comp; c0 += CT_GROUP, jobs += CT_JOBS) {
    const int nc = n_comp - c0 < CT_GROUP ? n_comp - c0 : CT_GROUP;
    int j0[CT_GROUP][CT_PER];
    float L[CT_GROUP][CT_PER][4];
    int jf[CT_GROUP];
    unsigned uni = 0;  // bit c: the whole wave sits on one stencil of component c
#pragma unroll
    for (int c = 0; c < CT_GROUP; ++c) {
      jf[c] = 0;
      if (c < nc) {
        const ContComp cc = comps[c0 + c];
        bool same = true;
#pragma unroll
        for (int j = 0; j < CT_PER; ++j) j0[c][j] = cont_stencil(cc, nu[j], L[c][j]);
        jf[c] = __builtin_amdgcn_readfirstlane(j0[c][0]);
#pragma unroll
        for (int j = 0; j < CT_PER; ++j) same = same && j0[c][j] == jf[c];
        uni |= (unsigned)__builtin_amdgcn_readfirstlane(__all(same)) << c;
      }
    }
    for (int l = 0; l < n_layers; ++l) {
      const float k = c2T[l], it = invT[l];
      float R[CT_PER], R_T[CT_PER];
#pragma unroll
      for (int j = 0; j < CT_PER; ++j) radiation_terms_d(nuf[j], nuf[j] * k, it, R[j], R_T[j]);
      ContJob nxt = jobs[0];
      for (int q = 0; nxt.mask != 0; ++q) {
        const ContJob job = nxt;
        nxt = jobs[q + 1];  // the list ends with a mask of 0: q + 1 < CT_JOBS
        const bool is_T = job.slot < 0;
        float* dst = (is_T ? dT + (size_t)l * (size_t)ld : K + ((size_t)job.slot * (size_t)n_layers + (size_t)l) * (size_t)ld) + (size_t)i0;
        const float* __restrict__ const tab_d = tab + (size_t)tab_stride * (is_T ? 1 : 2);  // dA/dT or dA/dMF, tab_stride after A
        float4 cur = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (full) cur = *reinterpret_cast<const float4*>(dst);
        float pos[CT_PER] = {0.0f, 0.0f, 0.0f, 0.0f}, acc[CT_PER] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < CT_GROUP; ++c) {
          if (job.mask >> c & 1) {
            const int r = ((c0 + c) * n_layers + l) * ld_nodes;  // fits an int with tab_stride (checked on the host)
            float s[CT_PER], sd[CT_PER];
            cont_sums(tab + r, (uni >> c & 1u) != 0, jf[c], j0[c], L[c], s);
            cont_sums(tab_d + r, (uni >> c & 1u) != 0, jf[c], j0[c], L[c], sd);
#pragma unroll
            for (int j = 0; j < CT_PER; ++j) {
              pos[j] += fmaxf(s[j], 0.0f);
              acc[j] += s[j] > 0.0f ? sd[j] : 0.0f;
            }
          }
        }
        float d[CT_PER];
#pragma unroll
        for (int j = 0; j < CT_PER; ++j) d[j] = is_T ? fmaf(R_T[j], pos[j], R[j] * acc[j]) : R[j] * acc[j];
        if (full) {
          cur.x += d[0];
          cur.y += d[1];
          cur.z += d[2];
          cur.w += d[3];
          *reinterpret_cast<float4*>(dst) = cur;
        } else {
          for (int j = 0; j < cnt; ++j) dst[j] += d[j];
        }
      }
    }
  }
}

extern "C" int rtx_continuum_add_d(const rtx_grid* grid, int n_layers, const double* T_h, int n_comp, const double* v0_h,
                                   const double* dv_h, const int32_t* n_nodes_h, const float* tables_h, const float* tables_dT_h,
                                   const float* tables_dx_h, int64_t ld_nodes, const int32_t* slot_h, int n_spec, float* dOD_dT,
                                   float* K, int64_t ld, void* stream, unsigned flags) {
  if (!grid || !T_h || !v0_h || !dv_h || !n_nodes_h || !tables_h || !slot_h) RTX_FAIL("a required pointer is NULL");
  if (flags != 0) RTX_FAIL("rtx_continuum_add_d: flags=%u, none is defined", flags);
  if (!dOD_dT && !K) RTX_FAIL("rtx_continuum_add_d: dOD_dT and K are both NULL");
  if (dOD_dT && !tables_dT_h) RTX_FAIL("rtx_continuum_add_d: dOD_dT needs tables_dT_h");
  if (rtx_check_grid(grid)) return 1;
  if (n_layers < 1 || n_comp < 1 || n_spec < 0) RTX_FAIL("n_layers=%d n_comp=%d n_spec=%d", n_layers, n_comp, n_spec);
  if (ld < grid->n) RTX_FAIL("ld=%lld smaller than n=%lld", (long long)ld, (long long)grid->n);
  if (ld_nodes < 4 || ld_nodes > 0x7fffffffLL) RTX_FAIL("ld_nodes=%lld", (long long)ld_nodes);
  bool any_slot = false;
  for (int c = 0; c < n_comp; ++c) {
    if (slot_h[c] < -1 || slot_h[c] >= n_spec) RTX_FAIL("slot_h[%d]=%d outside [-1, n_spec=%d)", c, (int)slot_h[c], n_spec);
    any_slot = any_slot || slot_h[c] >= 0;
  }
  if (any_slot && !K) RTX_FAIL("rtx_continuum_add_d: K is NULL but a component names a slot");
  if (any_slot && !tables_dx_h) RTX_FAIL("rtx_continuum_add_d: K needs tables_dx_h");
  float* const K_used = any_slot ? K : nullptr;
  const float* const tabs_h[3] = {tables_h, dOD_dT ? tables_dT_h : nullptr, K_used ? tables_dx_h : nullptr};
  static const char* const tab_name[3] = {"tables_h", "tables_dT_h", "tables_dx_h"};
  const int n_groups = (n_comp + CT_GROUP - 1) / CT_GROUP;
  const size_t jobs_off = (size_t)n_comp * sizeof(ContComp);
  const size_t c2T_off = jobs_off + (size_t)n_groups * CT_JOBS * sizeof(ContJob);
  std::vector<char> head(c2T_off + 2 * (size_t)n_layers * sizeof(float));  // zero-filled: every job list ends
  ContComp* const comps = (ContComp*)head.data();
  ContJob* const jobs = (ContJob*)(head.data() + jobs_off);
  for (int c0 = 0, gi = 0; c0 < n_comp; c0 += CT_GROUP, ++gi) {
    ContJob* job = jobs + (size_t)gi * CT_JOBS;
    const int nc = n_comp - c0 < CT_GROUP ? n_comp - c0 : CT_GROUP;
    if (dOD_dT) *job++ = ContJob{-1, (1 << nc) - 1};
    for (int c = 0; c < nc; ++c) {  // a slot's job at the first component of the group that names it
      const int sl = slot_h[c0 + c];
      bool first = sl >= 0;
      for (int b = 0; b < c; ++b) first = first && slot_h[c0 + b] != sl;
      if (!first) continue;
      int mask = 0;
      for (int b = c; b < nc; ++b)
        if (slot_h[c0 + b] == sl) mask |= 1 << b;
      *job++ = ContJob{sl, mask};
    }
  }
  float* const c2T = (float*)(head.data() + c2T_off);
  float* const invT = c2T + n_layers;
  for (int c = 0; c < n_comp; ++c) {
    const int nn = n_nodes_h[c];
    if (nn < 4 || nn > ld_nodes) RTX_FAIL("component %d: %d nodes (at least 4, at most ld_nodes=%lld)", c, nn, (long long)ld_nodes);
    if (!isfinite(v0_h[c]) || !isfinite(dv_h[c]) || !(dv_h[c] > 0.0)) RTX_FAIL("component %d: v0=%g dv=%g", c, v0_h[c], dv_h[c]);
    comps[c].v0 = v0_h[c];
    comps[c].dv = dv_h[c];
    comps[c].vend = v0_h[c] + (double)(nn - 1) * dv_h[c];
    comps[c].n = nn;
    comps[c].pad = 0;
    for (int t = 0; t < 3; ++t) {  // a non-finite node value would poison every point of its stencils
      if (!tabs_h[t]) continue;
      for (int l = 0; l < n_layers; ++l) {
        const float* const row = tabs_h[t] + ((size_t)c * (size_t)n_layers + (size_t)l) * (size_t)ld_nodes;
        for (int j = 0; j < nn; ++j)
          if (!isfinite(row[j])) RTX_FAIL("%s[%d][%d][%d] is not finite", tab_name[t], c, l, j);
      }
    }
  }
  for (int l = 0; l < n_layers; ++l) {
    if (!isfinite(T_h[l]) || !(T_h[l] > 0.0)) RTX_FAIL("T_h[%d]=%g", l, T_h[l]);
    c2T[l] = (float)(CT_C2 / T_h[l]);
    invT[l] = (float)(1.0 / T_h[l]);
  }
  if (grid->n == 0 || (!dOD_dT && !K_used)) return 0;
  if ((grid->n + CT_TILE - 1) / CT_TILE > 0x7fffffffLL) RTX_FAIL("n=%lld too large", (long long)grid->n);
  hipStream_t st = (hipStream_t)stream;
  const size_t head_bytes = (head.size() + 15) / 16 * 16;
  const size_t tab_floats = (size_t)n_comp * (size_t)n_layers * (size_t)ld_nodes;
  const size_t tab_stride = (tab_floats + 3) / 4 * 4;  // floats between the three tables, each 16-byte aligned
  if (3 * tab_stride > 0x7fffffffULL) RTX_FAIL("tables of %zu values each are too large", tab_floats);
  void* base = nullptr;
  if (g_cont_d_scratch->get(stream, head_bytes + 3 * tab_stride * sizeof(float), &base)) return 1;
  RTX_HIP(hipMemcpyAsync(base, head.data(), head.size(), hipMemcpyHostToDevice, st));  // pageable: staged before returning
  float* const tab_d = (float*)((char*)base + head_bytes);
  for (int t = 0; t < 3; ++t)  // a table the call does without is not staged, and not read
    if (tabs_h[t]) RTX_HIP(hipMemcpyAsync(tab_d + (size_t)t * tab_stride, tabs_h[t], tab_floats * sizeof(float), hipMemcpyHostToDevice, st));
  const ContComp* const comps_d = (const ContComp*)base;
  const ContJob* const jobs_d = (const ContJob*)((const char*)base + jobs_off);
  const float* const c2T_d = (const float*)((const char*)base + c2T_off);
  const float* const invT_d = c2T_d + n_layers;
  const unsigned tiles = (unsigned)((grid->n + CT_TILE - 1) / CT_TILE);
  const bool vec = (ld % 4 == 0) && (((uintptr_t)dOD_dT & 15) == 0) && (((uintptr_t)K_used & 15) == 0);
  if (vec)
    hipLaunchKernelGGL(continuum_add_d_kernel<true>, dim3(tiles), dim3(CT_BLOCK), 0, st, to_dev(grid), n_layers, n_comp, comps_d, jobs_d,
                       c2T_d, invT_d, tab_d, (int)tab_stride, (int)ld_nodes, dOD_dT, K_used, (long long)ld);
  else
    hipLaunchKernelGGL(continuum_add_d_kernel<false>, dim3(tiles), dim3(CT_BLOCK), 0, st, to_dev(grid), n_layers, n_comp, comps_d, jobs_d,
                       c2T_d, invT_d, tab_d, (int)tab_stride, (int)ld_nodes, dOD_dT, K_used, (long long)ld);
  RTX_LAUNCH_CHECK();
  return 0;
}
