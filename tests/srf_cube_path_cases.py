"""Every instantiation and every exit of the per-pixel HSI cube's derivative kernels (rtx_srf_pixel_cube_vjp, rtx_srf_pixel_cube_jvp,
rtx_srf_pixel_cube_normal, rtx_srf_pixel_cube_fit): the case lists, the host-side formulas of the three .hip files restated,
and the scenes and tables of the fit's exit cases, which tests/test_srf_cube_paths_host.py (CPU: every case does what its
name says, in the fp64 code alone) and tests/test_gpu_srf_cube_paths.py (the kernels) share. NumPy only, fixed seeds. The
oracles are those of srf_cube_vjp_cases, srf_cube_jvp_cases and srf_cube_fit_cases; nothing is restated of them.

The kernels are templates on the node count Q = 1 .. 8, the pixel kernels also on the table's placement (LDS when
nEnd * Q <= 128), the tangent on NV = 1, 2, the two fit kernels on nMix = 1 .. 4. One temperature range for every Q: the
comparisons are with the node form, so how well 1 or 2 nodes interpolate Planck's function does not enter.
"""
import numpy as np

import srf_cube_fit_cases as FT

T_RANGE = (285.0, 315.0)
NPIX = 65          # one full wave of the fit plus one pixel; one ragged round of 64 of the pixel kernels
Q_MAX = 8          # rtx_srf_cube_max_nodes()
MIX_MAX = 4        # rtx_srf_pixel_cube_fit_max_mix()
TAB_LDS = 128      # SC_TAB_LDS / SCV_TAB_LDS / SCJ_TAB_LDS / SCF_TAB_LDS
KNOTS = "coarse"

Q_LIST = tuple(range(1, Q_MAX + 1))
QMIX = tuple((Q, nMix) for Q in Q_LIST for nMix in range(1, MIX_MAX + 1))


def in_lds(nEnd, Q):
    return nEnd * Q <= TAB_LDS


def nend_list(Q):
    """5 (5 Q runs through every residue mod 4 over Q = 1 .. 8), the largest table in LDS, the smallest in global memory."""
    return (5, TAB_LDS // Q, TAB_LDS // Q + 1)


def fit_stride(nEnd, Q):
    """scf_front: words per band of the fit's LDS slice, nEnd * Q rounded up to an odd number of 16-byte pieces; 0: global memory."""
    return 4 * (((nEnd * Q + 3) // 4) | 1) if in_lds(nEnd, Q) else 0


VJP_CHUNK, VJP_WS_MAX = 256, 64 << 20  # SCV_CHUNK, SCV_WS_MAX


def vjp_chunks(nEnd, Q, nB, nPix):
    """rtx_srf_pixel_cube_vjp: (pixels per chunk of the reduction, chunks): 256, doubled until the chunks' fp64 sums
    [chunk][nEnd + 1][Q][nB] fit 64 MiB."""
    per_chunk = (nEnd + 1) * Q * nB * 8
    chunk = VJP_CHUNK
    n = lambda: (nPix + chunk - 1) // chunk
    while n() > 1 and n() * per_chunk > VJP_WS_MAX:
        chunk *= 2
    return chunk, n()


# section 3: band counts on both sides of one and of two blocks of 64, with the table in LDS and in global memory
NB_FIT = (1, 63, 64, 65, 128, 129)
NB_DERIV = (63, 64, 65, 129)
BLOCK_TABLES = ((8, 8), (5, 31))  # (Q, nEnd): 64 rows in LDS, 155 in global memory
BLOCK_SCALAR = (7, 2)             # (Q, nMix) of the fit in place of Q = 8: the scalar row read (Q % 4 != 0) across a block

# section 5: 400 endmembers of 8 nodes in 80 bands are 2 053 120 bytes per chunk, of which 64 MiB hold 32. 8193 pixels
# are the fewest with 33 chunks of 256: they become 17 of 512, the last of one pixel. 8449 pixels (34 chunks of 256) are 17 of
# 512 too, the last of 257: more than the 256 it would have held undoubled.
CHUNK_CASE = dict(nEnd=400, Q=8, nB=80, nPix=8193)
CHUNK_NPIX = (8193, 8449)
JVP_TILE_NEND = (63, 64)  # the re-layout kernel's nEnd + 1 columns: one tile of 64 exactly, and one column into a second

# section 4: the scene of the exit cases
EXIT = dict(Q=5, nEnd=8, nMix=3)
NOISE = 1e-3


def exit_scene(seed=5):
    return FT.distinct_scene(NPIX, EXIT["nMix"], EXIT["nEnd"], T_RANGE, seed=seed)


def end_scene(seed=5):
    """exit_scene with every true T on an end of the range, the two ends alternating (pixels 0 and 1 are there already)."""
    sc = exit_scene(seed)
    sc["T"] = np.asarray(T_RANGE, dtype=np.float64)[np.arange(NPIX) % 2]
    return sc


def noisy(cube, seed=37):
    """cube (1 + 1e-3 N(0, 1)), float32; a NaN (a dead band) stays one."""
    n = np.random.default_rng(seed).standard_normal(np.shape(cube))
    return (np.asarray(cube).astype(np.float64) * (1.0 + NOISE * n)).astype(np.float32)


def tie(tab, node_axis):
    """The table with every node's rows equal to node 0's: every node of the scan then gives the same cost."""
    tab = np.array(tab)
    first = np.take(tab, [0], axis=node_axis)
    tab[...] = first
    return tab


def nan_pixel(meas, live_band, pixel=17):
    """meas with one NaN, under a band that counts, in one pixel."""
    m = np.array(meas)
    m[live_band, pixel] = np.nan
    return m, pixel


def block_weights(nB=129, seed=33):
    """Weights in [0.5, 2) with zeros on bands 63 and 64 where they exist: the last band of a block and the first of the next."""
    w = np.random.default_rng(seed).uniform(0.5, 2.0, nB).astype(np.float32)
    w[[b for b in (63, 64) if b < nB]] = 0.0
    return w
