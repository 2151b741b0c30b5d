"""CPU-only checks of tests/srf_cube_path_cases.py: every case of tests/test_gpu_srf_cube_paths.py does what its name says, shown
with the fp64 code alone (srf_cube_fit_cases.fit with the kernel's fp32 roundings simulated) on the fp64 moments of the
"coarse" case rounded to float32, and with the library's own constants and source text."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from radtxfr_amd import _lib

import srf_cube_cases as CC
import srf_cube_fit_cases as FT
import srf_cube_path_cases as PC
import srf_fused_cases as FC

CSRC = os.path.join(ROOT, "radtxfr_amd", "csrc")


def _define(name, text):
    m = re.search(r"^#define\s+%s\s+(.+?)\s*(?://.*)?$" % name, text, flags=re.M)
    assert m, name
    return m.group(1)


def test_case_lists_cover_every_instantiation():
    """The (Q, nMix) list is the full product of the library's two limits (both entries answer without a device); every nEnd
    list has a table in LDS on one side of SC_TAB_LDS and one in global memory on the other, by the #defines of the four .hip
    files, which agree; 5 Q runs through every residue mod 4."""
    lib = _lib.load()
    QM, MM = lib.rtx_srf_cube_max_nodes(), lib.rtx_srf_pixel_cube_fit_max_mix()
    assert (QM, MM) == (PC.Q_MAX, PC.MIX_MAX)
    assert list(PC.QMIX) == [(Q, m) for Q in range(1, QM + 1) for m in range(1, MM + 1)] and len(PC.QMIX) == 32
    assert list(PC.Q_LIST) == list(range(1, QM + 1))
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("rtx_srf_cube.hip", "rtx_srf_cube_vjp.hip", "rtx_srf_cube_jvp.hip", "rtx_srf_cube_fit.hip")}
    lds = [int(_define(n, src[f])) for n, f in (("SC_TAB_LDS", "rtx_srf_cube.hip"), ("SCV_TAB_LDS", "rtx_srf_cube_vjp.hip"),
                                                ("SCJ_TAB_LDS", "rtx_srf_cube_jvp.hip"), ("SCF_TAB_LDS", "rtx_srf_cube_fit.hip"))]
    assert lds == [PC.TAB_LDS] * 4
    for Q in PC.Q_LIST:
        small, edge, over = PC.nend_list(Q)
        assert PC.in_lds(small, Q) and edge * Q <= PC.TAB_LDS < over * Q and over == edge + 1
        assert edge >= MM  # a scene of distinct endmembers fits the first `edge` columns
    assert {5 * Q % 4 for Q in PC.Q_LIST} == {0, 1, 2, 3}
    assert {(e * Q) % 4 for Q in PC.Q_LIST for e in PC.nend_list(Q) if PC.in_lds(e, Q)} == {0, 1, 2, 3}
    for Q, nEnd in PC.BLOCK_TABLES:
        assert Q in PC.Q_LIST
    assert PC.in_lds(PC.BLOCK_TABLES[0][1], PC.BLOCK_TABLES[0][0]) and not PC.in_lds(PC.BLOCK_TABLES[1][1], PC.BLOCK_TABLES[1][0])
    assert PC.BLOCK_SCALAR[0] % 4 != 0 and PC.in_lds(PC.BLOCK_TABLES[0][1], PC.BLOCK_SCALAR[0])
    for nbs in (PC.NB_FIT, PC.NB_DERIV):
        assert {63, 64, 65, 129} <= set(nbs)
    assert int(_define("SCV_CHUNK", src["rtx_srf_cube_vjp.hip"])) == PC.VJP_CHUNK
    assert _define("SCV_WS_MAX", src["rtx_srf_cube_vjp.hip"]) == "(64ll << 20)" and PC.VJP_WS_MAX == 64 << 20
    assert int(_define("SCF_PB", src["rtx_srf_cube_fit.hip"])) == PC.NPIX - 1


def test_restated_formulas():
    """The fit's stride is nEnd Q rounded up to an odd number of 16-byte pieces: the documented values at the shapes of the
    first test's cases, and 0 past the threshold. The adjoint's chunk: 256 until 33 chunks of [401][8][80] fp64 no longer fit 64
    MiB; the chosen scene is the smallest that doubles it, doubles it once, and ends in a ragged chunk."""
    assert [PC.fit_stride(5, Q) for Q in PC.Q_LIST] == [12, 12, 20, 20, 28, 36, 36, 44]
    assert PC.fit_stride(8, 8) == 68 and PC.fit_stride(16, 8) == 132 and PC.fit_stride(17, 8) == 0 and PC.fit_stride(18, 7) == 132
    for Q in PC.Q_LIST:
        for nEnd in PC.nend_list(Q):
            S = PC.fit_stride(nEnd, Q)
            assert (S == 0) == (not PC.in_lds(nEnd, Q))
            assert S == 0 or (S >= nEnd * Q and S % 4 == 0 and (S // 4) % 2 == 1 and S - nEnd * Q < 8 and S * 64 * 4 <= 64 << 10)
    c = PC.CHUNK_CASE
    assert PC.vjp_chunks(**c) == (512, 17) and c["nPix"] % 512 != 0 and PC.CHUNK_NPIX[0] == c["nPix"]
    assert [PC.vjp_chunks(**dict(c, nPix=n)) for n in PC.CHUNK_NPIX] == [(512, 17)] * 2 and [n % 512 for n in PC.CHUNK_NPIX] == [1, 257]
    assert PC.vjp_chunks(**dict(c, nPix=c["nPix"] - 1)) == (256, 32)
    assert PC.vjp_chunks(**dict(c, nPix=257)) == (256, 2)
    assert PC.vjp_chunks(**dict(c, nPix=32 * 512 + 1)) == (1024, 17)  # where it would double a second time
    assert PC.vjp_chunks(400, 8, 80, 257) == (256, 2) and PC.vjp_chunks(8, 8, 20, 65) == (256, 1)
    assert [n + 1 for n in PC.JVP_TILE_NEND] == [64, 65]


@pytest.fixture(scope="module")
def exits():
    """(N, Cb, G, Tq) of the exit cases' shape on the "coarse" case, rounded to float32 as the device holds them, the scene and
    the simulated forward's cube at its truth."""
    lib = _lib.load()
    c = FC.case(lib.rtx_srf_chunk_points(), lib.rtx_srf_max_knots(), PC.KNOTS)
    Tq = CC.nodes(PC.T_RANGE, PC.EXIT["Q"])
    N, Cb, M, _ = FC.moments(c["X"], c["tables"], c["tau"], c["La"], c["Ld"], c["Xk"], Tq)
    r32 = lambda x: np.asarray(x).astype(np.float32).astype(np.float64)
    args = (r32(N), r32(Cb), r32(M @ CC.endmembers(c["Xk"].size, PC.EXIT["nEnd"]).astype(np.float64)), Tq)

    def forward(sc):
        y = FT.evaluate(*args, sc["kidx"], sc["frac"], sc["T"], np.zeros((args[0].size, PC.NPIX)), f32=True)["y"].astype(np.float32)
        y[args[0] == 0.0] = np.nan
        return y
    sc = PC.exit_scene()
    return args, sc, forward(sc), forward


def _fit(args, sc, meas, **kw):
    with np.errstate(invalid="ignore"):
        return FT.fit(*args, PC.T_RANGE, sc["kidx"], meas, f32=True, **kw)


def test_exits_status_3(exits):
    """Zero weights: status 3 for all 65 from the scan, status 0 with cost 0.0 from a given start. One NaN under a counting
    band: status 3 for that pixel alone, from the scan and from a given start. One node: a given start away from the truth has
    H_00 = 0 and is given up after no trial."""
    args, sc, meas, _ = exits
    zero = np.zeros(args[0].size)
    r = _fit(args, sc, meas, w=zero, max_iter=10)
    assert np.all(r["status"] == 3) and np.all(r["n_iter"] == 0) and np.isnan(r["T"]).all() and np.isnan(r["cost"]).all()
    r = _fit(args, sc, meas, w=zero, start=(sc["T"], sc["frac"]), max_iter=10)
    assert np.all(r["status"] == 0) and np.all(r["cost"] == 0.0) and np.all(r["n_iter"] == 0)
    m2, px = PC.nan_pixel(meas, int(np.flatnonzero(args[0] > 0.0)[0]))
    assert np.isnan(m2[:, px]).sum() == np.isnan(meas[:, px]).sum() + 1
    for start in (None, (sc["T"], (sc["frac"] * np.float32(0.9)).astype(np.float32))):
        r = _fit(args, sc, m2, start=start, max_iter=10)
        assert np.array_equal(np.flatnonzero(r["status"] == 3), [px]) and np.all(r["status"][np.arange(PC.NPIX) != px] <= 1)
    one = (args[0], args[1], args[2][:1], CC.nodes(PC.T_RANGE, 1))
    r = _fit(one, sc, meas, start=(sc["T"], (sc["frac"] * np.float32(0.9)).astype(np.float32)), max_iter=10)
    assert np.all(r["status"] == 3) and np.all(r["n_iter"] == 0)


def test_exits_lambda_cap_clamp_and_tie(exits):
    """The noisy scene at ftol = 0: all 65 end with status 0 and a cost above 0 well before 200 trials, which only the cap of
    lambda does; a restart from the result at lambda0 = 1e11 stops after at most 2 trials where it is. With every true T on an
    end of the range, some final T is an end exactly. With every node's rows equal, the scan keeps node 0; without, it does not.
    MEASURED (fp64 NumPy, fp32 simulated): 15 to 41 trials on the noisy scene; 27 final temperatures on an end."""
    args, sc, meas, forward = exits
    mn = PC.noisy(meas)
    assert np.array_equal(np.isnan(mn), np.isnan(meas)) and not np.array_equal(mn, meas, equal_nan=True)
    r = _fit(args, sc, mn, max_iter=200, ftol=0.0)
    print("srf cube paths, noisy scene: trials %d .. %d" % (r["n_iter"].min(), r["n_iter"].max()))
    assert np.all(r["status"] == 0) and np.all(r["cost"] > 0.0) and r["n_iter"].max() < 200
    r2 = _fit(args, sc, mn, start=(r["T"], r["frac"]), max_iter=5, lambda0=1e11)
    assert np.all(r2["status"] == 0) and np.all(r2["n_iter"] <= 2) and np.array_equal(r2["T"], r["T"]) and np.array_equal(r2["frac"], r["frac"])
    se = PC.end_scene()
    assert np.all((se["T"] == PC.T_RANGE[0]) | (se["T"] == PC.T_RANGE[1])) and len(set(se["T"])) == 2
    r = _fit(args, se, PC.noisy(forward(se)), max_iter=200, ftol=0.0)
    on_end = (r["T"] == PC.T_RANGE[0]) | (r["T"] == PC.T_RANGE[1])
    print("srf cube paths, clamp scene: %d final temperatures on an end, trials %d .. %d" % (on_end.sum(), r["n_iter"].min(), r["n_iter"].max()))
    assert np.all(r["status"] == 0) and on_end.sum() >= 10 and not on_end.all()
    tied = (args[0], args[1], PC.tie(args[2], 0), args[3])
    assert np.array_equal(tied[2][3], args[2][0]) and not np.array_equal(args[2][3], args[2][0])
    r = _fit(tied, sc, meas, max_iter=0)
    assert np.all(r["status"] == 1) and np.all(r["T"] == args[3][0])
    r = _fit(args, sc, meas, max_iter=0)
    assert np.all(r["status"] == 1) and np.all(np.isin(r["T"], args[3])) and not np.all(r["T"] == args[3][0])
