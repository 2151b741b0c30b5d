// What the derivatives of the per-pixel cube and the fit built on them share (rtx_srf_cube_vjp.hip, rtx_srf_cube_jvp.hip,
// rtx_srf_cube_fit.hip): the node weights of a pixel.
#pragma once

// l_q(T) and l'_q(T) in fp64, the products over r ascending as rtx_srf_pixel_cube forms them, one division each.
// a.Tn: the nodes; a.den[q] = prod_{r != q} (T_q - T_r), r ascending, from the host (ScvArgs, ScjArgs).
template <int Q, class Args>
__device__ __forceinline__ void srf_cube_weight(const Args& a, double T, int q, double& l, double& dl) {
  double num = 1.0, dnum = 0.0;
#pragma unroll
  for (int r = 0; r < Q; ++r)
    if (r != q) num *= T - a.Tn[r];
#pragma unroll
  for (int s = 0; s < Q; ++s) {
    if (s == q) continue;
    double prod = 1.0;
#pragma unroll
    for (int r = 0; r < Q; ++r)
      if (r != q && r != s) prod *= T - a.Tn[r];
    dnum += prod;
  }
  l = num / a.den[q];
  dl = dnum / a.den[q];
}
