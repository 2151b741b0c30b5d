"""tud_g_kernel's pass over the layers an opaque column hides (RTX_TUD_OD_NONNEG, rtx_tud.hip), path by path.

Hand-built float32 columns go through rtx_tud_opts with the flag on and off. Every case is held to the fp64 oracle
(cpu_ref.tud_from_od) at the tolerances of tests/test_gpu_tud_paths.py -- 1e-5 relative for L-up and L-down, 2e-6 absolute
for tau -- and to the same call with the flag off: tau and L-down bit for bit, L-up within 2^-35 B_hot at the point's own
wavenumber (cases that must stay on the full pass: all three bit for bit).

Which path a wave took does not show in the outputs, so the cases force it by construction and prove it by poison: with the
flag on, a NaN written into layers the design says the wave never loads must leave every output bit unchanged, and a NaN in
a layer it does load must not. The numbers the columns are built around, on the grid used here (900 cm^-1, 205..295 K):
opaque_y = 27 + log2(B_hot / B_cold) ~ 30, so the downwelling stops looking once a lane's depth passes ~21, the top counts
as opaque from a depth of (opaque_y + 8) / log2(e) ~ 26.3, and tau is exactly 0 from a depth of 151 / log2(e) ~ 104.7.
Decisions are per wave of 64 points and on chunks of 4 layers; a wave looks only if its downwelling died (or ran out of
layers) within the first chunk, and then at 12 layers (3 chunks) from the top.

The L-up bound against the flag-off run is the design's bound on what is dropped BEFORE rounding; it lies 2^-11 ulp below
L-up, so it asks for equal bits except where that sliver moves a rounding (bench.py's dump: 2 of 4 000 000 points, by one
ulp). The hand-built columns are opaque far beyond the threshold (or exactly at t = 0), where nothing is left to move a
rounding; the real-table case has 4000 points, about 0.2 % odds of holding such a point, and its seeded table and window
hold none (the figures are printed with -s).

n = 200 and 640 (whole waves and a ragged last one, rows padded to a wider leading dimension); 5 layers (too few for a
chunk to be saved: the flag must change nothing), 32, and 70 (second Planck register set, ragged top chunk)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cpu_ref as ref
from radtxfr_amd import synthetic

pytestmark = pytest.mark.gpu

TOL_L = 1e-5
TOL_TAU = 2e-6
STAGE, SCAN = 4, 12
LO, STEP = 900.0, 0.001
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THIN = 0.01   # a layer that neither output notices much
D_DEAD = 24.0  # a depth past which the downwelling has stopped looking (~21 here)
D_TOP = 30.0   # a depth that makes the top opaque (~26.3 here)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib, engine
    _lib.load()
    return engine


def _rel(got, want):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    den = np.maximum(np.maximum(np.abs(want), 1e-3 * float(np.max(np.abs(want)))), 1e-30)
    return float(np.max(np.abs(got - want) / den))


def _temps(nL):
    T = np.linspace(295.0, 205.0, nL)
    if nL >= 8:
        T[nL // 4:nL // 4 + 2] = (250.0, 262.0)  # an inversion
    return T


def _run(eng, OD, T, n_down=None, mask=None, flag=True, returnOD=False, pad=7):
    """rtx_tud_opts on OD [nL][n] (rows padded by `pad` floats): (tau, Lu, Ld) as float32 host arrays."""
    import ctypes as C

    import torch
    from radtxfr_amd import _lib
    nL, n = OD.shape
    grid = eng.Grid(LO, LO + STEP * (n - 1), n)
    buf = torch.full((nL, n + pad), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :n] = torch.as_tensor(OD)
    mask = np.ones(nL, dtype=np.uint8) if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    n_down = int(mask.sum()) if n_down is None else n_down
    out = torch.empty((3, n + pad), dtype=torch.float32, device="cuda")
    T_h = np.ascontiguousarray(T, dtype=np.float64)
    mu = np.ones(1)
    vp = C.c_void_p
    _lib.check(_lib.load().rtx_tud_opts(vp(buf.data_ptr()), buf.stride(0), grid.byref(), nL, T_h.ctypes.data_as(vp), 1,
                                        mask.ctypes.data_as(vp), 1, mu.ctypes.data_as(vp), n_down, 30, int(returnOD),
                                        vp(out[0].data_ptr()), vp(out[1].data_ptr()), vp(out[2].data_ptr()), None, n + pad,
                                        vp(torch.cuda.current_stream().cuda_stream), 1 if flag else 0))
    res = out[:, :n].cpu().numpy()
    return res[0], res[1], res[2]


def _oracle(OD, T, n_down=None, mask=None, returnOD=False):
    nL, n = OD.shape
    X = LO + STEP * np.arange(n)
    mask = np.ones(nL, bool) if mask is None else np.asarray(mask, bool)
    Z = np.where(mask, 1.0, 9.0)
    tau, Lu, Ld = ref.tud_from_od(X, OD.astype(np.float64).T, T, Z, Altitudes=(5.0,), returnOD=returnOD)
    if n_down is not None and n_down != int(mask.sum()):  # the downwelling over the first n_down layers alone
        Zd = np.where(np.arange(nL) < n_down, 1.0, 9.0)
        Ld = ref.tud_from_od(X, OD.astype(np.float64).T, T, Zd, Altitudes=(5.0,))[2]
    return tau, Lu, Ld


def _b_hot(n, T):
    X = LO + STEP * np.arange(n)
    return ref.planckian(X, np.array([float(np.max(T))]))[:, 0]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check(eng, OD, T, same_bits=False, rows=slice(None), **kw):
    """Flag on against the oracle and against flag off. same_bits: the points `rows` must keep all three outputs."""
    on, off = _run(eng, OD, T, flag=True, **kw), _run(eng, OD, T, flag=False, **kw)
    tr, ur, dr = _oracle(OD, T, **kw)
    fin = np.isfinite(OD).all(0)
    tag = (OD.shape, kw)
    if kw.get("returnOD"):
        assert _rel(on[0][fin], tr[fin]) <= TOL_L, tag
    else:
        assert np.max(np.abs(on[0][fin].astype(np.float64) - tr[fin])) <= TOL_TAU, tag
    assert _rel(on[1][fin], ur[fin]) <= TOL_L, tag
    assert _rel(on[2][fin], dr[fin]) <= TOL_L, tag
    assert np.array_equal(_bits(on[0]), _bits(off[0])), tag
    assert np.array_equal(_bits(on[2]), _bits(off[2])), tag
    d = np.abs(on[1].astype(np.float64) - off[1].astype(np.float64))[fin]
    print("L-up on/off: %d of %d points differ, worst %.3g of the bound" % (
        np.count_nonzero(d), d.size, float(np.max(d / (2.0 ** -35 * _b_hot(OD.shape[1], T)[fin]))) if d.size else 0.0))
    assert np.all(d <= 2.0 ** -35 * _b_hot(OD.shape[1], T)[fin]), tag
    if same_bits:
        assert np.array_equal(_bits(on[1])[rows], _bits(off[1])[rows]), tag
    return on, off


def _unread(eng, OD, T, layers, on, **kw):
    """With the flag on the wave must not load `layers`: NaN there leaves every output bit where it was."""
    P = OD.copy()
    P[layers] = np.nan
    got = _run(eng, P, T, flag=True, **kw)
    for a, b in zip(got, on):
        assert np.array_equal(_bits(a), _bits(b)), (OD.shape, layers)


def _read(eng, OD, T, layer, **kw):
    """... and it does load `layer`: NaN there reaches tau."""
    P = OD.copy()
    P[layer] = np.nan
    assert np.isnan(_run(eng, P, T, flag=True, **kw)[0]).all(), (OD.shape, layer)


def _thin(rng, nL, n):
    return (THIN * rng.uniform(0.5, 1.5, (nL, n))).astype(np.float32)


def _k_top(nL):
    return (nL - 1) // STAGE * STAGE


SHAPES = [(5, 200), (32, 200), (32, 640), (70, 640)]


@pytest.mark.parametrize("nL,n", SHAPES)
def test_opaque_everywhere_skips_the_middle_unread(eng, nL, n):
    rng = np.random.default_rng(1)
    OD = rng.uniform(50.0, 70.0, (nL, n)).astype(np.float32)
    T = _temps(nL)
    on, _ = _check(eng, OD, T, same_bits=nL == 5)
    assert np.all(on[0] == 0.0)
    if nL > 5:  # bottom chunk, then straight to the top chunk: 4 x 50 + the top put tau at 0 without the middle
        _unread(eng, OD, T, slice(STAGE, _k_top(nL)), on)
        _read(eng, OD, T, STAGE - 1)
        _read(eng, OD, T, _k_top(nL))


@pytest.mark.parametrize("nL,n", SHAPES)
def test_opaque_ends_thin_middle_is_summed_for_tau(eng, nL, n):
    rng = np.random.default_rng(2)
    OD = _thin(rng, nL, n)
    T = _temps(nL)
    OD[0] = D_DEAD * rng.uniform(1.0, 1.1, n)
    OD[nL - 1] = D_TOP * rng.uniform(1.0, 1.1, n)
    on, _ = _check(eng, OD, T, same_bits=nL == 5)
    assert np.all(on[0] > 0.0) and np.all(on[0] < 1e-20)  # depth ~55: far below 104.7, tau a normal float32
    if nL > 5:
        _read(eng, OD, T, STAGE + 1)  # the middle is in the sum, bit for bit (above), so it was loaded
        # ... until the sum passes 104.7 in every lane: a thick layer in the second chunk ends the summing after that chunk
        OD[STAGE + 2] = 90.0
        on, _ = _check(eng, OD, T)
        assert np.all(on[0] == 0.0)
        if _k_top(nL) > 2 * STAGE:
            _unread(eng, OD, T, slice(2 * STAGE, _k_top(nL)), on)


@pytest.mark.parametrize("nL,n", SHAPES)
def test_one_transparent_lane_keeps_its_wave_on_the_full_pass(eng, nL, n):
    rng = np.random.default_rng(3)
    OD = rng.uniform(50.0, 70.0, (nL, n)).astype(np.float32)
    T = _temps(nL)
    OD[:, 64 + 17] = 1e-3  # one point of the second wave sees through the column
    on, _ = _check(eng, OD, T, same_bits=True, rows=slice(64, 128))
    if nL > 5:
        P = OD.copy()
        P[STAGE:_k_top(nL), 64:128] = np.nan  # that wave reads its middle, the others do not read theirs
        P[STAGE:_k_top(nL), 0:64] = np.nan
        got = _run(eng, P, T, flag=True)
        assert np.isnan(got[0][64:128]).all() and np.array_equal(_bits(got[0][:64]), _bits(on[0][:64]))
        assert np.array_equal(_bits(got[1][:64]), _bits(on[1][:64]))


@pytest.mark.parametrize("nL,n", SHAPES)
def test_thin_column_and_opaque_bottom_alone_change_nothing(eng, nL, n):
    rng = np.random.default_rng(4)
    T = _temps(nL)
    OD = _thin(rng, nL, n)
    _check(eng, OD, T, same_bits=True)   # the downwelling lives to the top: never scans
    OD[0] = 60.0
    _check(eng, OD, T, same_bits=True)   # dies at once, the scan runs its 12 layers and finds nothing
    if nL > 5:
        OD[_k_top(nL) - SCAN] = D_TOP    # opaque from one chunk below the scan limit: still nothing
        _check(eng, OD, T, same_bits=True)
        _read(eng, OD, T, _k_top(nL) - SCAN + 1)


@pytest.mark.parametrize("nL,n", SHAPES[1:])
def test_resume_chunk_first_scanned_and_at_the_scan_limit(eng, nL, n):
    rng = np.random.default_rng(5)
    T = _temps(nL)
    kt = _k_top(nL)
    for k_res in (kt, kt - STAGE, kt - (SCAN - STAGE)):
        OD = _thin(rng, nL, n)
        OD[0] = 120.0  # bottom + top past 104.7: nothing in between is loaded
        m = min(STAGE, nL - k_res)
        OD[k_res:k_res + m] = (D_TOP / m) * rng.uniform(1.0, 1.2, (m, n))  # opaque as a whole chunk only
        on, _ = _check(eng, OD, T)
        assert np.all(on[0] == 0.0)
        _unread(eng, OD, T, slice(STAGE, k_res), on)
        _read(eng, OD, T, k_res)


@pytest.mark.parametrize("nL,n", SHAPES[1:])
def test_downwelling_dying_after_the_first_chunk_does_not_look(eng, nL, n):
    """Thin first chunk, an opaque layer in the second, an opaque top: the wave stays on the full pass."""
    rng = np.random.default_rng(6)
    T = _temps(nL)
    OD = _thin(rng, nL, n)
    OD[STAGE + 1] = D_DEAD + 100.0
    OD[nL - 1] = D_TOP
    _check(eng, OD, T, same_bits=True)
    _read(eng, OD, T, _k_top(nL) - 2)


@pytest.mark.parametrize("nL,n", [(8, 200), (9, 200), (12, 200)])
def test_nothing_or_one_chunk_between_bottom_and_top(eng, nL, n):
    """8 layers: the bottom chunk ends where the top chunk begins, nothing to skip. 9 (ragged top chunk) and 12: one chunk."""
    rng = np.random.default_rng(10)
    OD = rng.uniform(50.0, 70.0, (nL, n)).astype(np.float32)
    T = _temps(nL)
    on, _ = _check(eng, OD, T, same_bits=nL == 8)
    if nL == 8:
        _read(eng, OD, T, STAGE + 1)
    else:
        _unread(eng, OD, T, slice(STAGE, 2 * STAGE), on)
        _read(eng, OD, T, 2 * STAGE)


@pytest.mark.parametrize("nL,n", SHAPES)
def test_return_od_and_non_prefix_mask_stay_on_the_full_pass(eng, nL, n):
    rng = np.random.default_rng(7)
    OD = rng.uniform(50.0, 70.0, (nL, n)).astype(np.float32)
    T = _temps(nL)
    _check(eng, OD, T, same_bits=True, returnOD=True)
    mask = np.ones(nL, np.uint8)
    mask[1] = 0
    mask[nL - 1] = 0  # count nL - 2 with a hole: tau sums the mask, L-up runs over the first nL - 2 layers
    on = _run(eng, OD, T, mask=mask, n_down=nL - 2, flag=True)
    off = _run(eng, OD, T, mask=mask, n_down=nL - 2, flag=False)
    for a, b in zip(on, off):
        assert np.array_equal(_bits(a), _bits(b))
    tr, ur, dr = _oracle(OD, T, mask=mask)  # (n_down = the mask's count: the oracle's own quirk)
    assert np.max(np.abs(on[0].astype(np.float64) - tr)) <= TOL_TAU
    assert _rel(on[1], ur) <= TOL_L and _rel(on[2], dr) <= TOL_L
    if nL > 5:
        _read(eng, OD, T, STAGE + 1, mask=mask, n_down=nL - 2)


@pytest.mark.parametrize("nL,n", SHAPES)
def test_downwelling_over_no_layer_and_over_fewer_than_the_count(eng, nL, n):
    rng = np.random.default_rng(8)
    T = _temps(nL)
    OD = _thin(rng, nL, n)
    OD[nL - 1] = D_TOP + 100.0
    for n_down in (0, 2):
        on, _ = _check(eng, OD, T, same_bits=nL == 5, n_down=n_down)
        if n_down == 0:
            assert np.all(on[2] == 0.0)
        if nL > 5:  # the downwelling is out of layers after the first chunk: the scan starts there
            _unread(eng, OD, T, slice(STAGE, _k_top(nL)), on, n_down=n_down)


@pytest.mark.parametrize("nL,n", SHAPES[1:])
def test_nan_depths(eng, nL, n):
    rng = np.random.default_rng(9)
    T = _temps(nL)
    OD = rng.uniform(50.0, 70.0, (nL, n)).astype(np.float32)
    # in a scanned top layer, flag on: the comparison fails, that wave stays on the full pass and the NaN shows as before
    P = OD.copy()
    P[nL - 2, 70] = np.nan
    on, off = _check(eng, P, T, same_bits=True, rows=slice(64, 128))
    assert np.isnan(on[0][70]) and np.isnan(on[1][70]) and np.isnan(off[0][70]) and np.isnan(off[1][70])
    assert np.array_equal(_bits(on[1][64:128]), _bits(off[1][64:128]))
    # in a middle layer, flag off: poisons tau and L-up of its point as before, and no other
    P = OD.copy()
    P[nL // 2, 70] = np.nan
    off = _run(eng, P, T, flag=False)
    clean = _run(eng, OD, T, flag=False)
    assert np.isnan(off[0][70]) and np.isnan(off[1][70])
    keep = np.arange(n) != 70
    for a, b in zip(off, clean):
        assert np.array_equal(_bits(a)[keep], _bits(b)[keep])


@pytest.mark.parametrize("nL,n", [(32, 200), (32, 640)])
def test_engine_tud_keyword(eng, nL, n):
    """The same through engine.tud(od_nonneg=): keyword off is rtx_tud, keyword on skips (poison), also from the blocks of
    slant paths a call with more than TUD_MAX_MU of them is cut into (every block a single-altitude call of 8 or 1 pairs:
    only the last, single pair can skip)."""
    import torch
    rng = np.random.default_rng(11)
    OD = rng.uniform(50.0, 70.0, (nL, n)).astype(np.float32)
    T = _temps(nL)
    Z = np.arange(nL, dtype=np.float64)
    grid = eng.Grid(LO, LO + STEP * (n - 1), n)
    P = OD.copy()
    P[STAGE:_k_top(nL)] = np.nan

    def run(od, theta=0.0, **kw):
        res = eng.tud(torch.as_tensor(od, device="cuda"), grid, T, Z, Altitudes=(500,), theta_r=theta, **kw)
        return [t.cpu().numpy() for t in res[:3]]

    off, on, default = run(OD, od_nonneg=False), run(OD, od_nonneg=True), run(OD)
    direct_on, direct_off = _run(eng, OD, T, flag=True, pad=0), _run(eng, OD, T, flag=False, pad=0)
    for a, b, c, d, e in zip(on, off, default, direct_on, direct_off):
        assert np.array_equal(_bits(a).ravel(), _bits(d).ravel()) and np.array_equal(_bits(b).ravel(), _bits(e).ravel())
        assert np.array_equal(_bits(b), _bits(c))
    poisoned = run(P, od_nonneg=True)
    for a, b in zip(poisoned, on):
        assert np.array_equal(_bits(a), _bits(b))
    assert np.isnan(run(P, od_nonneg=False)[0]).all()
    # nine slant paths: a block of eight (never skips) and a block of one (skips with the keyword)
    theta = np.linspace(0.0, 0.8, 9)
    t9, u9, _ = run(P, theta=theta, od_nonneg=True)
    assert np.isnan(t9[:8]).all() and np.isfinite(t9[8]).all() and np.isfinite(u9[8]).all()
    assert np.isnan(run(P, theta=theta)[0]).all()


_CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
from test_gpu_tud_skip import _compute_tud_cases
np.savez(sys.argv[2], **_compute_tud_cases())
"""


def _compute_tud_cases():
    """rtx_compute_tud (TudRunner) on a 4 cm^-1 window of the C3 table at full mixing ratios, an opaque column: as it is,
    and with one negative mixing ratio (a negative column weight: the library must not vouch for the optical depths)."""
    import torch
    from radtxfr_amd import engine
    full = synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
    lo, hi, n = 1000.0, 1004.0, 4000  # cpu_ref.make_spectral_axis(1000, 1004, 0.001)
    sub = synthetic.subset_table(full, lo - 12.0, hi + 12.0)
    a = synthetic.c3_atmosphere(32)
    lines = engine.LineTable(sub)
    grid = engine.Grid(lo, hi, n)
    out = {}
    for name, mf in (("real", a["MFs_VAL"]), ("negative", np.where(np.arange(32)[:, None] == 20, -a["MFs_VAL"], a["MFs_VAL"]))):
        run = engine.TudRunner(lines, grid, a["Zs"], n_layers=32)
        tau, Lu, Ld = run.run(a["Ts"], a["Ps"], a["PLs"], mf, a["MFs_ID"])
        torch.cuda.synchronize()
        out.update({name + "_tau": tau.cpu().numpy(), name + "_Lu": Lu.cpu().numpy(), name + "_Ld": Ld.cpu().numpy()})
    return out


def test_compute_tud_switch_on_and_off(tmp_path):
    import torch
    assert torch.cuda.is_available()
    assert os.environ.get("RADTXFR_TUD_SKIP") != "0", "this test compares the default with RADTXFR_TUD_SKIP=0"
    on = _compute_tud_cases()
    path = str(tmp_path / "off.npz")
    env = dict(os.environ, RADTXFR_TUD_SKIP="0")
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], check=True, env=env, timeout=300)
    off = np.load(path)
    for k in ("negative_tau", "negative_Lu", "negative_Ld", "real_tau", "real_Ld"):
        assert np.array_equal(_bits(on[k]), _bits(off[k])), k
    X = ref.make_spectral_axis(1000.0, 1004.0, 0.001)
    a = synthetic.c3_atmosphere(32)
    b_hot = ref.planckian(X, np.array([float(np.max(a["Ts"]))]))[:, 0]
    d = np.abs(on["real_Lu"].astype(np.float64) - off["real_Lu"].astype(np.float64)).ravel()
    print("compute_tud L-up on/off: %d of %d points differ, worst %.3g of the bound" % (np.count_nonzero(d), d.size, float(np.max(d / (2.0 ** -35 * b_hot)))))
    assert np.all(d <= 2.0 ** -35 * b_hot)
    full = synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
    sub = synthetic.subset_table(full, 1000.0 - 12.0, 1004.0 + 12.0)
    _, tr, ur, dr = ref.compute_TUD(sub, 1000.0, 1004.0, 0.001, a["Zs"], a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"])
    assert np.max(np.abs(on["real_tau"].ravel() - tr)) <= TOL_TAU
    assert _rel(on["real_Lu"].ravel(), ur) <= TOL_L and _rel(on["real_Ld"].ravel(), dr) <= TOL_L
