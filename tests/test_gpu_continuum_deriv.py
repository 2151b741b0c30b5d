"""GPU: derivatives through the tabulated continuum (rtx_continuum_add_d, engine.continuum_add_d, continuum_derivatives=True
of the five derivative drop-ins). The kernel point by point against the float64 definition
(continuum.Continuum.dod_host) at the project's pin of 1e-5 of the row's largest value, its bit-level properties (cuts of the
axis, the in-place add, the mask of rtx_continuum_add), the refusals and the stream contract of the entry, and the drop-ins
end to end: J against the oracle's closed-form chain rule fed line derivatives + dod_host, the adjoint and the tangent against
that J, the band radiances' adjoint identity.

With RADTXFR_CONTINUUM_DERIV_PROFILE=<file> the module writes the worst error of every kernel case to that file
(profiles/continuum_deriv_accuracy.txt is such a file); the bound is asserted either way."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import continuum_cases as K
import continuum_deriv_cases as D
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL_SPECIES = 2e-4   # tests/test_gpu_jacobian.py
TOL_T = 2e-3         # tests/test_gpu_jacobian.py
TOL_L = 1e-5         # tests/test_gpu_tud_jvp.py
U32 = 2.0 ** -24
F32_TINY = 2.0 ** -126
F32_FLOOR = 1e-30    # tests/test_gpu_tud_jvp.py
NEAR_KINK = 1e-4     # points with |S| < NEAR_KINK sum_k |L_k A_k| in float64 are left out: float32 may see the other sign
_ROWS = []
LISTS = ("one", "two", "shared", "skip", "five")


@pytest.fixture(scope="module")
def mods():
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib, continuum, engine, sensor, synthetic
    from radtxfr_amd import radiative_transfer as rt
    m = dict(lib=_lib.load(), _lib=_lib, ct=continuum, engine=engine, sensor=sensor, synthetic=synthetic, rt=rt)
    assert int(m["lib"].rtx_continuum_tile_points()) == 1024  # N_AXIS = two tiles + 3, the n below sit around one tile
    yield m
    path = os.environ.get("RADTXFR_CONTINUUM_DERIV_PROFILE")
    if path and _ROWS:
        with open(path, "w") as f:
            f.write("# tests/test_gpu_continuum_deriv.py::test_kernel_point_by_point, written by the module itself with\n"
                    "# RADTXFR_CONTINUUM_DERIV_PROFILE=<this file> (%s, torch %s).\n"
                    "# worst |device - dod_host| / max|dod_host of the row| over the rows of a case (dOD/dT: the layers; dOD/dMF:\n"
                    "# the layers of every slot); asserted <= %.0e\n"
                    "# grid | components | layers | n | ld | dOD/dT | dOD/dMF\n"
                    % (torch.cuda.get_device_name(0), torch.__version__, K.TOL_PIN))
            for r in _ROWS:
                f.write(r + "\n")
            f.write("# worst of all cases: dOD/dT %.3g, dOD/dMF %.3g\n"
                    % (max(float(r.split("|")[5]) for r in _ROWS), max(float(r.split("|")[6]) for r in _ROWS)))


def _largs(lay):
    return lay["T"], lay["P"], lay["PL"], lay["MF"], lay["ID"]


def _near_kink(sums):
    """[nL][nX]: some component's float64 stencil sum lies within NEAR_KINK of 0, relative to its terms, inside its axis."""
    near = False
    for S, M, ins in sums:
        near = near | (ins[None, :] & (np.abs(S) < NEAR_KINK * M))
    return near


@pytest.fixture(scope="module")
def refs(mods):
    """Per (grid, layers, component list), on the whole axis, made once and read-only: the Continuum, the species of K's
    slots, the layers, dod_host's dOD/dT [nL][nX] and dOD/dMF [nS][nL][nX] in slot order, `near` [nL][nX] the points left
    out (some component's float64 stencil sum within NEAR_KINK of 0 relative to its terms), `dead_T` / `dead_K` the points
    where no component that adds to the output has a positive stencil sum."""
    out = {}
    for name in K.GRIDS:
        X = mods["engine"].Grid(*K.grid_args(name)).axis()
        lists = D.component_lists(mods["ct"], name)
        for nL in (1, 3):
            lay = K.layers(nL)
            for key, (cont, species) in lists.items():
                dT, dMF = cont.dod_host(X, *_largs(lay))
                # a molecule's entry sums all its components; "skip" leaves a molecule out of K altogether
                dK = np.stack([dMF[m] for m in species])
                sums = D.stencil_sums(cont, X, *_largs(lay))
                near = _near_kink(sums)
                dead_T = np.ones((nL, X.size), dtype=bool)
                dead_K = np.ones((len(species), nL, X.size), dtype=bool)
                inside = np.zeros(X.size, dtype=bool)
                for c, (S, M, ins) in zip(cont.components, sums):
                    dead_T &= ~(S > 0.0)
                    if c.molecule in species:
                        dead_K[species.index(c.molecule)] &= ~(S > 0.0)
                    inside |= ins
                assert near[:, inside].mean() <= 0.01
                for a in (dT, dK, near, dead_T, dead_K):
                    a.setflags(write=False)
                out[(name, nL, key)] = dict(cont=cont, species=species, lay=lay, dT=dT, dK=dK, near=near, dead_T=dead_T, dead_K=dead_K)
    return out


def _blocks(nL, nS, n, aligned, fill_T=None, fill_K=None):
    """Float32 views dOD_dT [nL][n] and K [nS][nL][n] with one row stride: aligned -- rows 16 bytes apart from 16-byte aligned
    bases; not aligned -- an odd leading dimension from bases one float past such an address."""
    ld = (n + 3) // 4 * 4 if aligned else (n + 4) // 4 * 4 + 1
    pad = 0 if aligned else 1
    bT = torch.zeros(nL * ld + 4, dtype=torch.float32, device="cuda")
    bK = torch.zeros(nS * nL * ld + 4, dtype=torch.float32, device="cuda")
    dT = bT[pad:][:nL * ld].view(nL, ld)[:, :n]
    Kb = bK[pad:][:nS * nL * ld].view(nS, nL, ld)[:, :, :n]
    assert (dT.data_ptr() % 16 == 0) == aligned and (Kb.data_ptr() % 16 == 0) == aligned and (ld % 4 == 0) == aligned
    if fill_T is not None:
        dT.copy_(torch.as_tensor(fill_T, device="cuda"))
    if fill_K is not None:
        Kb.copy_(torch.as_tensor(fill_K, device="cuda"))
    return dT, Kb


def _run(mods, r, grid, dT, Kb):
    return mods["engine"].continuum_add_d(r["cont"], grid, *_largs(r["lay"]), dOD_dT=dT, K=Kb, species=r["species"])


def _worst(got, want, keep):
    """Worst |got - want| over the points kept, relative to each row's largest |want| on the whole axis."""
    scale = np.max(np.abs(want[0]), axis=-1, keepdims=True)
    assert np.all(scale > 0.0)
    return float(np.max(np.where(keep, np.abs(got - want[1]), 0.0) / scale))


@pytest.mark.parametrize("aligned", [True, False], ids=["ld4", "ld_odd"])
@pytest.mark.parametrize("n", [1, 3, 1024, 1027, 2051])
@pytest.mark.parametrize("key", LISTS)
@pytest.mark.parametrize("nL", [1, 3])
@pytest.mark.parametrize("name", sorted(K.GRIDS))
def test_kernel_point_by_point(mods, refs, name, nL, key, n, aligned):
    """From zeroed blocks the device result against dod_host at every point that is not within NEAR_KINK of a kink: at most
    1e-5 of the row's largest value; exactly 0.0 where no contributing component has a positive stencil sum. The calls with
    one output left out give the bits of the call with both."""
    r = refs[(name, nL, key)]
    nS = len(r["species"])
    grid = mods["engine"].Grid(*K.grid_args(name))
    off = 0 if n == K.N_AXIS else 5  # a run that does not start on a multiple of 4 of the axis
    g = grid.shard(off, n)
    dT, Kb = _blocks(nL, nS, n, aligned)
    _run(mods, r, g, dT, Kb)
    got_T, got_K = dT.double().cpu().numpy(), Kb.double().cpu().numpy()
    sl = slice(off, off + n)
    keep = ~r["near"][:, sl]
    assert np.all(np.isfinite(got_T)) and np.all(np.isfinite(got_K))
    e_T = _worst(got_T, (r["dT"], r["dT"][:, sl]), keep)
    e_K = _worst(got_K, (r["dK"], r["dK"][:, :, sl]), keep[None])
    print("%s %s nL=%d n=%d %s: worst error dOD/dT %.3g, dOD/dMF %.3g of the row maximum (bound %.0e)"
          % (name, key, nL, n, "ld % 4 == 0" if aligned else "odd ld", e_T, e_K, K.TOL_PIN))
    _ROWS.append("%-6s | %-6s | %d | %4d | %4d | %.3g | %.3g" % (name, key, nL, n, dT.stride(0) if nL > 1 else n, e_T, e_K))
    assert e_T <= K.TOL_PIN and e_K <= K.TOL_PIN
    assert np.all(got_T[r["dead_T"][:, sl] & keep] == 0.0) and np.all(got_K[r["dead_K"][:, :, sl] & keep[None]] == 0.0)
    only_T, _ = _blocks(nL, nS, n, aligned)
    _, only_K = _blocks(nL, nS, n, aligned)
    _run(mods, r, g, only_T, None)
    _run(mods, r, g, None, only_K)
    assert torch.equal(only_T, dT) and torch.equal(only_K, Kb)


@pytest.mark.parametrize("aligned", [True, False], ids=["ld4", "ld_odd"])
@pytest.mark.parametrize("key", LISTS)
@pytest.mark.parametrize("name", sorted(K.GRIDS))
def test_cuts_are_bit_identical(mods, refs, name, key, aligned):
    """Ragged shards of the axis at odd offsets give the bits of the uncut call."""
    r = refs[(name, 3, key)]
    nS = len(r["species"])
    grid = mods["engine"].Grid(*K.grid_args(name))
    full_T, full_K = _blocks(3, nS, K.N_AXIS, True)
    _run(mods, r, grid, full_T, full_K)
    assert float(full_T.abs().max()) > 0 and float(full_K.abs().max()) > 0
    for a, b in ((0, 1021), (1021, 1539), (1539, K.N_AXIS), (1023, 1024)):
        assert a == 0 or a % 2 == 1
        dT, Kb = _blocks(3, nS, b - a, aligned)
        _run(mods, r, grid.shard(a, b - a), dT, Kb)
        assert torch.equal(dT, full_T[:, a:b]), (a, b, int((dT != full_T[:, a:b]).sum()))
        assert torch.equal(Kb, full_K[:, :, a:b]), (a, b, int((Kb != full_K[:, :, a:b]).sum()))


@pytest.mark.parametrize("aligned", [True, False], ids=["ld4", "ld_odd"])
@pytest.mark.parametrize("key", ["one", "two", "shared", "skip"])
@pytest.mark.parametrize("name", sorted(K.GRIDS))
def test_in_place_add(mods, refs, name, key, aligned):
    """With at most four components (one register group) the result on a random non-zero block is float32(block) + (the
    result from zeros), bit for bit: each destination row is read and written once, the group's terms summed first."""
    r = refs[(name, 3, key)]
    nS, n = len(r["species"]), K.N_AXIS
    grid = mods["engine"].Grid(*K.grid_args(name))
    pure_T, pure_K = _blocks(3, nS, n, aligned)
    _run(mods, r, grid, pure_T, pure_K)
    pT, pK = pure_T.cpu().numpy(), pure_K.cpu().numpy()
    rng = np.random.default_rng(12)
    b_T = (rng.uniform(-1.0, 1.0, pT.shape) * np.abs(pT).max(axis=-1, keepdims=True)).astype(np.float32)  # of the derivative's size
    b_K = (rng.uniform(-1.0, 1.0, pK.shape) * np.abs(pK).max(axis=-1, keepdims=True)).astype(np.float32)
    assert np.all(b_T != 0.0) and np.all(b_K != 0.0)
    dT, Kb = _blocks(3, nS, n, aligned, fill_T=b_T, fill_K=b_K)
    _run(mods, r, grid, dT, Kb)
    assert np.array_equal((b_T + pT).view(np.uint32), dT.cpu().numpy().view(np.uint32))
    assert np.array_equal((b_K + pK).view(np.uint32), Kb.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("which", [0, 1], ids=["full", "steps"])
@pytest.mark.parametrize("name", sorted(K.GRIDS))
def test_the_mask_is_the_one_rtx_continuum_add_applied(mods, name, which):
    """One component at a time: where rtx_continuum_add, from zeros, left 0.0 both derivatives are 0.0; where it left
    something the mask is set (dOD/dMF is not 0 there). "steps" on the coarse grid is cut by max(0, .) on part of its axis."""
    eng = mods["engine"]
    m, v0, dv, nn, kind = K.GRIDS[name]["comps"][which]
    cont = K.component(mods["ct"], m, v0, dv, nn, seed=3 + which, kind=kind)
    lay = K.layers(3)
    grid = eng.Grid(*K.grid_args(name))
    od = torch.zeros((3, K.N_AXIS), dtype=torch.float32, device="cuda")
    eng.continuum_add(cont, grid, *_largs(lay), od)
    dT, Kb = _blocks(3, 1, K.N_AXIS, False)
    eng.continuum_add_d(cont, grid, *_largs(lay), dOD_dT=dT, K=Kb, species=(m,))
    zero = od == 0.0
    assert bool(zero.any()) == (which == 1) and bool((~zero).any())
    assert bool((dT[zero] == 0.0).all()) and bool((Kb[0][zero] == 0.0).all())
    assert bool((Kb[0][~zero] != 0.0).all())
    if name == "coarse" and which == 1:
        X = grid.axis()
        inside = (X >= v0) & (X <= cont.components[0].vend)
        assert int(zero[:, torch.as_tensor(inside, device="cuda")].sum()) > 0  # cut inside the axis, not only outside it


def test_entry_refusals(mods):
    eng, lib, _lib = mods["engine"], mods["lib"], mods["_lib"]
    lay = K.layers(3)
    cont = K.continuum(mods["ct"], "fine", 1)
    grid = eng.Grid(*K.grid_args("fine"))
    dT, Kb = _blocks(3, 1, K.N_AXIS, True)
    with pytest.raises(ValueError, match="molecule 1 is not in MF_ID"):
        eng.continuum_add_d(cont, grid, lay["T"], lay["P"], lay["PL"], lay["MF"], np.array([3, 2]), dOD_dT=dT)
    with pytest.raises(ValueError, match="both None"):
        eng.continuum_add_d(cont, grid, *_largs(lay))
    with pytest.raises(ValueError, match="species"):
        eng.continuum_add_d(cont, grid, *_largs(lay), K=Kb, species=(1, 2))
    dT, Kb = _blocks(1, 2, 8, True)
    T, v0, dv = np.array([280.0]), np.array([5989.0, 5989.0]), np.array([0.5, 0.5])
    nn = np.array([8, 8], dtype=np.int32)
    tab = np.ones((2, 1, 8), dtype=np.float32)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    dp = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(slots=(0, 1), n_spec=2, tabs=(tab, tab, tab), out=(dT, Kb), ld=8, flags=0, T=T, dv=dv, nn=nn):
        slots = np.array(slots, dtype=np.int32)
        return lib.rtx_continuum_add_d(grid.shard(0, 8).byref(), 1, vp(T), 2, vp(v0), vp(dv), vp(nn), vp(tabs[0]), vp(tabs[1]), vp(tabs[2]),
                                       8, vp(slots), n_spec, dp(out[0]), dp(out[1]), ld, eng._stream_ptr(), flags)
    bad = tab.copy()
    bad[1, 0, 5] = np.nan
    refused = [call(slots=(0, 2)), call(slots=(-2, 0)), call(slots=(0, 1), n_spec=1),       # slots outside [-1, n_spec)
               call(ld=7),                                                                  # ld < n
               call(tabs=(bad, tab, tab)), call(tabs=(tab, bad, tab)), call(tabs=(tab, tab, bad)),
               call(out=(None, None)), call(flags=1),
               call(out=(dT, None)),                                                        # a slot named, no K
               call(tabs=(tab, tab, None)), call(tabs=(tab, None, tab)),                    # an output without its table
               call(T=np.array([0.0])), call(dv=np.array([0.5, 0.0])), call(nn=np.array([8, 9], dtype=np.int32))]
    assert all(rc != 0 for rc in refused), refused
    with pytest.raises(_lib.RtxError, match="not finite"):
        _lib.check(call(tabs=(tab, tab, bad)))
    with pytest.raises(_lib.RtxError, match="both NULL"):
        _lib.check(call(out=(None, None)))
    torch.cuda.synchronize()
    assert float(dT.abs().max()) == 0.0 and float(Kb.abs().max()) == 0.0  # a refused call enqueues nothing
    # what is allowed: slot -1 everywhere without K and its table, no dOD_dT without its table, n = 0
    assert call(slots=(-1, -1), n_spec=0, tabs=(tab, tab, None), out=(dT, None)) == 0
    assert call(tabs=(tab, None, tab), out=(None, Kb)) == 0
    assert lib.rtx_continuum_add_d(grid.shard(0, 0).byref(), 1, vp(T), 2, vp(v0), vp(dv), vp(nn), vp(tab), vp(tab), vp(tab), 8,
                                   vp(np.array([0, 1], dtype=np.int32)), 2, dp(dT), dp(Kb), 8, eng._stream_ptr(), 0) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dT).all()) and float(dT.abs().min()) > 0.0 and float(Kb.abs().min()) > 0.0


# ---- the stream contract of rtx_continuum_add_d (include/radtxfr_hip.h), as tests/test_gpu_continuum.py holds rtx_continuum_add
# ---- to it: on a side stream that is busy when the call is made ---------------------------------------------------------------
def _stream_case(mods, v):
    """Variants 0, 1, 2: other layers, component lists, axis cuts and sizes. The two blocks are the payload (NaN until the
    stream has passed the delay, so a kernel that runs early adds to NaN); T, the axes, the slots and the three tables are
    the host arrays."""
    import stream_cases as S
    eng, lib, _lib = mods["engine"], mods["lib"], mods["_lib"]
    name, nL, key, off, n = (("fine", 3, "two", 0, K.N_AXIS), ("coarse", 1, "one", 5, 700), ("coarse", 2, "five", 1021, 333))[v]
    lay = K.layers(nL)
    lay["T"] = lay["T"] + 1.5 * v
    cont, species = D.component_lists(mods["ct"], name)[key]
    A, A_T, A_x, axes = cont.layer_tables_d(*_largs(lay))
    nC, nS = len(axes), len(species)
    grid = eng.Grid(*K.grid_args(name)).shard(off, n)
    slots = np.array([species.index(c.molecule) if c.molecule in species else -1 for c in cont.components], dtype=np.int32)
    host = dict(T=np.ascontiguousarray(lay["T"]), v0=np.array([x[0] for x in axes]), dv=np.array([x[1] for x in axes]),
                nn=np.array([x[2] for x in axes], dtype=np.int32), A=np.ascontiguousarray(A), A_T=np.ascontiguousarray(A_T),
                A_x=np.ascontiguousarray(A_x), slots=slots)
    rng = np.random.default_rng(80 + v)
    b_T = S.dev(rng.uniform(-1.0, 1.0, (nL, n)).astype(np.float32) * 1e-3)
    b_K = S.dev(rng.uniform(-1.0, 1.0, (nS, nL, n)).astype(np.float32) * 1e-5)

    def call(d, h):
        _lib.check(lib.rtx_continuum_add_d(grid.byref(), nL, S.hp(h["T"]), nC, S.hp(h["v0"]), S.hp(h["dv"]), S.hp(h["nn"]), S.hp(h["A"]),
                                           S.hp(h["A_T"]), S.hp(h["A_x"]), A.shape[2], S.hp(h["slots"]), nS, S.vp(d["dT"]), S.vp(d["K"]),
                                           n, eng._stream_ptr(), 0))
        return [d["dT"], d["K"]]
    # what the staging run writes into the host arrays once the call has returned: other finite values and valid slots, so
    # that a copy read late would change the bits without handing the kernel a stencil or a row outside its arrays
    scribble = dict(T=host["T"] + 40.0, v0=host["v0"] + 1.0, dv=host["dv"] * 1.5, nn=np.full(nC, 4, dtype=np.int32), A=A * 3.0 + 1.0,
                    A_T=A_T * 2.0 - 1.0, A_x=A_x * 0.5 + 1.0, slots=np.zeros(nC, dtype=np.int32))
    return S.Case(call, inputs={"dT": b_T, "K": b_K}, host=host, scribble=scribble), (b_T, b_K), (cont, species, lay, grid)


@pytest.fixture(scope="module")
def stream_env(mods):
    import stream_cases as S
    e = dict(S=S, s1=torch.cuda.Stream(), s2=torch.cuda.Stream(), delay=S.Delay())
    yield e
    torch.cuda.synchronize()


def test_stream_order_asynchrony_and_staging(mods, stream_env):
    """Behind a delay on s1, with the blocks NaN until s1 has passed the delay, the call gives the default-stream bits; the
    warmed call returns while the delay is pending; the host arrays may be overwritten as soon as it has returned. The
    default-stream result is block + dod_host within the pin."""
    S, s1, delay = stream_env["S"], stream_env["s1"], stream_env["delay"]
    case, (b_T, b_K), (cont, species, lay, grid) = _stream_case(mods, 0)
    other, _, _ = _stream_case(mods, 1)
    ref, _ = S.run_plain(case)
    w_T, w_M = cont.dod_host(grid.axis(), *_largs(lay))
    w_K = np.stack([w_M[m] for m in species])
    near = _near_kink(D.stencil_sums(cont, grid.axis(), *_largs(lay)))  # beside a kink float32 may see the other sign
    assert near.mean() <= 0.01
    for got, blk, want in ((ref[0], b_T, w_T), (ref[1], b_K, w_K)):
        b = blk.double().cpu().numpy()
        bound = K.TOL_PIN * np.abs(want).max(axis=-1, keepdims=True) + U32 * np.abs(b + want)  # the pin and the sum's rounding
        err = np.abs(S.as_float(got).astype(np.float64) - b - want)
        assert np.all((err <= bound) | near)
    warm, _ = S.run_plain(case, s1)   # grows the scratch of s1
    warm2, host_ms = S.run_plain(case, s1)
    Dms = delay.ms_for(host_ms, "rtx_continuum_add_d")
    S.run_plain(other, s1)            # the scratch of s1 now holds another call's tables
    out, pend, _ = S.run_delayed([case], s1, delay, Dms)
    S.run_plain(other, s1)
    out_s, pend_s, _ = S.run_delayed([case], s1, delay, Dms, scribble=True)
    torch.cuda.synchronize()
    print("rtx_continuum_add_d: returned before the delay had passed %s / %s, warmed host time %.3f ms, D %.0f ms"
          % (pend[0], pend_s[0], host_ms, Dms))
    for what, r in (("warm-up on s1", warm), ("warmed call on s1", warm2), ("behind the delay", out[0]), ("host arrays overwritten", out_s[0])):
        assert S.same_bits(r, ref), "%s: %s" % (what, S.describe(r, ref))
    assert pend[0] and pend_s[0], "the call returned only after %.0f ms of device work ahead of it on its stream had finished" % Dms


def test_two_calls_behind_one_delay_and_two_streams(mods, stream_env):
    """Delay, call A, call B (other tables, another size) on s1: each equals its solo reference, so B's tables did not reach
    A's kernel. Then delay and A on s1, B at once on s2, C on s1: the scratch is owned per (device, stream)."""
    S, s1, s2, delay = stream_env["S"], stream_env["s1"], stream_env["s2"], stream_env["delay"]
    cases = [_stream_case(mods, v)[0] for v in range(3)]
    refs_ = [S.run_plain(c)[0] for c in cases]
    assert not S.same_bits(refs_[0], refs_[1])
    host_ms = 0.0
    for st in (s1, s2):
        for c in cases:
            S.run_plain(c, st)
        host_ms = sum(S.run_plain(c, st)[1] for c in cases)
    Dms = delay.ms_for(host_ms, "rtx_continuum_add_d")
    out, _, _ = S.run_delayed(cases[:2], s1, delay, Dms)
    torch.cuda.synchronize()
    assert S.same_bits(out[0], refs_[0]), "A: " + S.describe(out[0], refs_[0])
    assert S.same_bits(out[1], refs_[1]), "B: " + S.describe(out[1], refs_[1])
    work = [S.fresh(c) for c in cases]
    torch.cuda.synchronize()
    res = [None, None, None]
    with torch.cuda.stream(s1):
        delay.enqueue(Dms)
        for i in (0, 2):
            S.fill(cases[i], work[i][0])
        res[0] = [x.clone() for x in S.flatten(S.issue(cases[0], *work[0])[0])]
    with torch.cuda.stream(s2):
        S.fill(cases[1], work[1][0])
        res[1] = [x.clone() for x in S.flatten(S.issue(cases[1], *work[1])[0])]
    with torch.cuda.stream(s1):
        res[2] = [x.clone() for x in S.flatten(S.issue(cases[2], *work[2])[0])]
    torch.cuda.synchronize()
    got = [S.finish(c, r) for c, r in zip(cases, res)]
    for nm, g, w in zip("ABC", got, refs_):
        assert S.same_bits(g, w), "%s: %s" % (nm, S.describe(g, w))


# ---- end to end: the drop-ins with continuum_derivatives=True --------------------------------------------------------------
XMIN, XMAX, DV = 1000.0, 1002.0, 0.01
H = 0.01           # tests/test_gpu_jacobian_dT.py: the step of the oracle's fixed-window difference of the line-sum
WRT = ("T", 1, 2)
ALTS = np.array([1.2, 500.0])  # between the layers and above them all
FD_STEP = 0.5      # the default fd_step_T of the drop-ins
THIN = 1e-3        # the mixing ratios of the "thin" column, as a fraction of the "full" one's


def _e2e_case(mods, mf_scale):
    """The synthetic line table and four-layer column of tests/test_gpu_continuum.py on 200 points, its mixing ratios times
    mf_scale; a continuum of a "full" component on H2O and a "steps" component on CO2 over part of the axis, each scaled
    to a column optical depth of about 0.25 whatever mf_scale; and the oracle in float64, made once: the total optical
    depth (line-sum + od_host), the line-sum's derivatives as tests/test_gpu_jacobian.py and tests/test_gpu_jacobian_dT.py
    build theirs (1 ppmv of one species; fixed-window central difference at +- H) plus dod_host, and J = g dOD + h from
    cpu_ref.jacobian_from_od. J_fd is the same with dOD/dT the central difference of the oracle's own optical depths
    (fixed-window line-sum + od_host) at +- FD_STEP: what dT_method="fd" is defined to compute, in exact arithmetic."""
    from oracle import cpu_ref
    rt, ct = mods["rt"], mods["ct"]
    tbl = mods["synthetic"].synth_line_table(20261019, 400, XMIN - 5.0, XMAX + 5.0)
    a = dict(DVOUT=DV, Zs=np.array([0.5, 1.5, 2.5, 3.5]), PLs=np.array([1.0, 1.0, 1.0, 1.0]),
             MFs_VAL=mf_scale * np.array([[8.0, 0.4], [5.0, 0.4], [2.0, 0.39], [1.0, 0.38]]), MFs_ID=np.array([1, 2]),
             Ts=np.array([290.0, 277.7, 263.1, 251.0]), Ps=np.array([95000.0, 70000.0, 50000.0, 31000.0]))
    X = rt.make_spectral_axis(XMIN, XMAX, DV)
    lay = (a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"])
    comps = []
    for unit in (K.component(ct, 1, 950.0, 10.0, 12, seed=6), K.component(ct, 2, 1000.303, 0.25, 9, seed=7, kind="steps")):
        s = 0.25 / unit.od_host(X, *lay).sum(axis=0).max()  # the definition is linear in the coefficients
        c = unit.components[0]
        comps.append(ct.Component(c.molecule, c.v0, c.dv, Cs_a=s * c.Cs_a, T_a=c.T_a, Cs_b=s * c.Cs_b, T_b=c.T_b, Cf=s * c.Cf))
    cont = ct.Continuum(comps)
    nL = 4
    od_c = cont.od_host(X, *lay)
    cut = ct.Continuum(comps[1:]).od_host(X, *lay)[:, (X >= comps[1].v0) & (X <= comps[1].vend)]
    assert np.any(cut == 0.0) and np.any(cut > 0.0)  # max(0, .) cuts inside the second axis
    od_l = np.stack([cpu_ref.layer_od(tbl, X, a["Ts"][k], a["Ps"][k], a["PLs"][k], a["MFs_VAL"][k], a["MFs_ID"]) for k in range(nL)])

    def window_difference(step):
        return np.stack([(cpu_ref.od_fixed_window(tbl, X, a["Ts"][k] + step, a["Ts"][k], a["Ps"][k], a["PLs"][k], a["MFs_VAL"][k], a["MFs_ID"])
                          - cpu_ref.od_fixed_window(tbl, X, a["Ts"][k] - step, a["Ts"][k], a["Ps"][k], a["PLs"][k], a["MFs_VAL"][k], a["MFs_ID"]))
                         / (2.0 * step) for k in range(nL)])
    d_T, d_MF = cont.dod_host(X, *lay)
    lines_T = window_difference(H)
    dOD = {"T": lines_T + d_T}
    lines_share = np.abs(lines_T).max() / np.abs(d_T).max()
    for col, m in enumerate((1, 2)):
        unit = np.zeros(2)
        unit[col] = 1.0
        dOD[m] = np.stack([cpu_ref.layer_od(tbl, X, a["Ts"][k], a["Ps"][k], a["PLs"][k], unit, a["MFs_ID"]) for k in range(nL)]) + d_MF[m]
    dOD_fd = window_difference(FD_STEP) + (cont.od_host(X, a["Ts"] + FD_STEP, *lay[1:]) - cont.od_host(X, a["Ts"] - FD_STEP, *lay[1:])) / (2.0 * FD_STEP)
    OD = (od_l + od_c).T  # [nX][nL]
    J, J_fd = {}, {}
    for returnOD in (False, True):
        g, h = cpu_ref.jacobian_from_od(X, OD, a["Ts"], a["Zs"], ALTS, returnOD=returnOD)  # [2 nZ + 1][nX][nL]
        J[returnOD] = {w: g * dOD[w].T[None] + (h if w == "T" else 0.0) for w in WRT}
        J_fd[returnOD] = g * dOD_fd.T[None] + h
    return dict(tbl=tbl, a=dict(a, Altitudes=ALTS), X=X, cont=cont, J=J, J_fd=J_fd, nL=nL, lines_share=lines_share)


def _worst_rows(got_rows, want, nL, exact_zeros=True):
    """Worst rel_err (floor 1e-3 of the row's maximum) over rows [2 nZ + 1] and layers; a (row, layer) the oracle has all
    zero (a layer above the sensor) must be all zero."""
    errs = []
    for row, got in enumerate(got_rows):
        for l in range(nL):
            if not np.any(want[row][:, l]):
                assert not exact_zeros or not np.any(got[:, l]), (row, l)
                continue
            errs.append(rel_err(got[:, l], want[row][:, l], floor_frac=1e-3))
    return max(errs)


@pytest.fixture(scope="module")
def e2e(mods):
    """_e2e_case at full mixing ratios: line optical depths up to 13 in the lowest layer, tau from 2e-9 to 0.35."""
    return _e2e_case(mods, 1.0)


@pytest.fixture(scope="module")
def e2e_thin(mods):
    """_e2e_case with the mixing ratios times THIN: the continuum is the larger part of the opacity (the window case), the
    lines' dOD/dT at its peak a sixth of the continuum's, 80 times TOL_T. This is the column on which dT_method="fd" can be held to the oracle's derivative:
    "fd" is DEFINED as a central difference at +- 0.5 K, and in float64 that difference of the oracle's own optical depths
    is off the oracle's derivative by 2.95e-3 on the full column (its lines' lower-state energies make the third derivative
    in T large), more than TOL_T, whatever computes it; on this column by 3.1e-5. The fixture asserts that this figure, which
    comes from the oracle alone, leaves three quarters of TOL_T to the code under test."""
    e = _e2e_case(mods, THIN)
    own = _worst_rows(e["J_fd"][False], e["J"][False]["T"], e["nL"])
    print("thin column: the 0.5 K central difference of the oracle against its derivative, float64: %.3e" % own)
    assert own <= 0.25 * TOL_T and e["lines_share"] >= 0.1
    return e


def _kw(e, **more):
    return dict(dict(line_table=e["tbl"], continuum=e["cont"], continuum_derivatives=True, **e["a"]), **more)


def _jacobian_rows(Jw, nZ):
    return [Jw[0][:, z, :] for z in range(nZ)] + [Jw[1][:, z, :] for z in range(nZ)] + [Jw[2]]


@pytest.mark.parametrize("method,column,returnOD", [("fd", "thin", False), ("analytic", "thin", False), ("analytic", "full", False),
                                                    ("analytic", "full", True)],
                         ids=["fd-thin", "analytic-thin", "analytic-full", "analytic-full-returnOD"])
def test_jacobian_against_the_oracle(mods, e2e, e2e_thin, method, column, returnOD):
    """J of compute_TUD_jacobian(continuum=, continuum_derivatives=True) against the oracle at the bounds of
    tests/test_gpu_jacobian.py (TOL_SPECIES for a species, TOL_T for "T"), row by row and layer by layer; the base outputs
    are compute_TUD(continuum=)'s bits. "fd" is held to the oracle's derivative on the thin column (e2e_thin says why); on the full
    one it is held to the "analytic" route at the band radiances (test_fd_and_analytic_routes_agree).

    MEASURED on an MI355X: "fd" thin T 4.7e-5, species 5.9e-7 and 2.2e-6; "analytic" thin T 9.8e-7; "analytic" full T 1.7e-5,
    species 2.4e-5 and 3.0e-5, the same under returnOD."""
    rt, e = mods["rt"], e2e if column == "full" else e2e_thin
    nZ = ALTS.size
    Xj, tau, Lu, Ld, J = rt.compute_TUD_jacobian(XMIN, XMAX, wrt=WRT, dT_method=method, **_kw(e, returnOD=returnOD))
    base = rt.compute_TUD(XMIN, XMAX, line_table=e["tbl"], continuum=e["cont"], returnOD=returnOD, **e["a"])
    for x, y in zip((Xj, tau, Lu, Ld), base):
        assert np.array_equal(x, y)
    plain = rt.compute_TUD_jacobian(XMIN, XMAX, wrt=WRT, dT_method=method, line_table=e["tbl"], returnOD=returnOD, **e["a"])[4]
    for w in WRT:
        want = e["J"][returnOD][w]
        tol = TOL_T if w == "T" else TOL_SPECIES
        worst = _worst_rows(_jacobian_rows(J[w], nZ), want, e["nL"])
        print("%s, %s column, returnOD=%s, wrt %r: worst rel_err against the oracle %.3e (bound %.0e)" % (method, column, returnOD, w, worst, tol))
        assert worst <= tol
        # the continuum must matter: without it the same entry misses the oracle
        assert rel_err(plain[w][1][:, nZ - 1, 0], want[2 * nZ - 1][:, 0], floor_frac=1e-3) > 10.0 * tol, w


def test_vjp_and_jvp_are_the_contractions_of_that_jacobian(mods, e2e):
    rt, e = mods["rt"], e2e
    kw = _kw(e, dT_method="analytic")
    X, nL, nZ = e["X"], e["nL"], ALTS.size
    nX = X.size
    _, tau, La, Ld, J = rt.compute_TUD_jacobian(XMIN, XMAX, wrt=WRT, **kw)
    rng = np.random.default_rng(5)
    n_vec = 2
    g_tau, g_La, g_Ld = rng.normal(size=(nX, nZ, n_vec)), rng.normal(size=(nX, nZ, n_vec)), rng.normal(size=(nX, n_vec))
    Xv, tau_v, La_v, Ld_v, grad = rt.compute_TUD_vjp(XMIN, XMAX, {"tau": g_tau, "La": g_La, "Ld": g_Ld}, wrt=WRT, **kw)
    for x, y in zip((Xv, tau_v, La_v, Ld_v), (X, tau, La, Ld)):
        assert np.array_equal(x, y)
    G32 = lambda g: g.astype(np.float32).astype(np.float64)  # the cotangent the device is given
    for w in WRT:
        dtau, dLa, dLd = J[w]
        terms = [("xav,xal->lv", G32(g_tau), dtau), ("xav,xal->lv", G32(g_La), dLa), ("xv,xl->lv", G32(g_Ld), dLd)]
        want = sum(np.einsum(s, g, j) for s, g, j in terms)
        scale = sum(np.einsum(s, np.abs(g), np.abs(j)) for s, g, j in terms)
        g_sum = np.abs(G32(g_tau)).sum(axis=(0, 1)) + np.abs(G32(g_La)).sum(axis=(0, 1)) + np.abs(G32(g_Ld)).sum(axis=0)
        bound = 4.0 * U32 * scale + F32_TINY * g_sum[None, :]  # tests/test_gpu_tud_vjp.py's bound
        err = np.abs(grad[w] - want)
        print("vjp vs stored J, wrt %r: worst |got - ref| / bound = %.3g" % (w, float(np.max(err / bound))))
        assert np.count_nonzero(want) == want.size and np.all(err <= bound), w
    tang = {"T": rng.normal(size=(nL, n_vec)), 1: rng.normal(size=(nL, n_vec)) * 0.5, 2: rng.normal(size=(nL, n_vec)) * 0.05}
    Xv, tau_v, La_v, Ld_v, d = rt.compute_TUD_jvp(XMIN, XMAX, tang, **kw)
    for x, y in zip((Xv, tau_v, La_v, Ld_v), (X, tau, La, Ld)):
        assert np.array_equal(x, y)
    for i_, name in enumerate(("tau", "La", "Ld")):
        sub_x = "xal,lv->xav" if name != "Ld" else "xl,lv->xv"
        want = sum(np.einsum(sub_x, J[w][i_], tang[w]) for w in WRT)
        S_J = 0.0
        for w in WRT:
            Jw = np.abs(J[w][i_])
            den = np.maximum(np.maximum(Jw, 1e-3 * np.max(Jw, axis=0, keepdims=True)), F32_FLOOR)
            S_J = S_J + np.einsum(sub_x, den, np.abs(tang[w]))
        v_sum = sum(np.abs(tang[w]).sum(axis=0) for w in WRT)
        bound = 2.0 * TOL_L * S_J + F32_TINY * v_sum + U32 * np.abs(want)  # tests/test_gpu_tud_jvp.py, end to end
        err = np.abs(d[name] - want)
        print("jvp vs stored J, %s: worst |got - ref| / bound = %.3g" % (name, float(np.max(err / bound))))
        assert np.count_nonzero(want) > 0.5 * want.size and np.all(err <= bound), name


def _band_case(mods, e):
    s = mods["sensor"].Sensor.from_shape([1000.40, 1000.95, 1001.50], 0.3, "triangle")
    Xk = np.array([999.9, 1000.5, 1001.0, 1001.5, 1002.1])
    rng = np.random.default_rng(9)
    E = rng.uniform(0.6, 1.0, (5, 3)).astype(np.float32)
    return s, Xk, E, 296.0, rng


def test_band_radiance_adjoint_identity(mods, e2e):
    """<g, J v> = <J^T g, v> at the band radiances under continuum_derivatives=True, within the sum of the two chains'
    bounds as tests/test_gpu_sensor_jvp.py::test_compute_band_radiance_jvp_end_to_end forms it: the sensor tangent's and the
    sensor adjoint's on the device rows, and through the stored Jacobian the TUD tangent's under |G| and the TUD adjoint's
    under |v|."""
    import sensor_jvp_cases as JC
    import sensor_vjp_cases as VC
    from test_gpu_sensor_vjp import K_DE, K_DTS, K_ROW
    rt, eng, sensor, e = mods["rt"], mods["engine"], mods["sensor"], e2e
    s, Xk, E, Ts_s, rng = _band_case(mods, e)
    kw = _kw(e, dT_method="analytic", Altitudes=np.array([500.0]))
    nL, nB, nk, nE, n_vec = e["nL"], 3, 5, 3, 2
    atm = {"T": rng.normal(size=(nL, n_vec)), 1: rng.normal(size=(nL, n_vec)) * 0.5, 2: rng.normal(size=(nL, n_vec)) * 0.05}
    surf = {"Ts_surface": rng.normal(size=n_vec), "emis": (rng.normal(size=(nk, nE, n_vec)) * 0.05).astype(np.float32)}
    X_out, L, dL = rt.compute_band_radiance_jvp(XMIN, XMAX, s, Xk, E, Ts_s, dict(atm, **surf), **kw)
    assert L.shape == (nB, nE) and dL.shape == (nB, nE, n_vec) and np.all(np.isfinite(L)) and np.all(np.isfinite(dL))
    cot = rng.normal(size=(nB, nE, n_vec)).astype(np.float32)
    _, L_v, grad = rt.compute_band_radiance_vjp(XMIN, XMAX, s, Xk, E, Ts_s, cot, wrt=WRT, **kw)
    assert np.array_equal(L, L_v)
    # L carries the continuum: it is band_radiance_srf_fused on compute_TUD(continuum=)'s outputs
    X, tau, La, Ld = rt.compute_TUD(XMIN, XMAX, line_table=e["tbl"], continuum=e["cont"], **dict(e["a"], Altitudes=np.array([500.0])))
    nX = X.size
    grid = eng.Grid(XMIN, XMAX, nX)
    dev32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float32), device="cuda")
    t_d, a_d, d_d, E_d = dev32(tau), dev32(La), dev32(Ld), dev32(E)
    _, L_f = sensor.band_radiance_srf_fused(grid, t_d, a_d, d_d, Xk, E_d, Ts_s, s)
    assert np.array_equal(L, L_f.cpu().numpy())
    _, _, _, _, rows = rt.compute_TUD_jvp(XMIN, XMAX, atm, **kw)
    r32 = {k: rows[k].astype(np.float32) for k in ("tau", "La", "Ld")}
    _, _, _, _, J = rt.compute_TUD_jacobian(XMIN, XMAX, wrt=WRT, **kw)  # {w: (dtau, dLa, dLd)}, each [nX][nL]
    tables = [(np.asarray(x), np.asarray(r)) for x, r in s.tables]
    names = ("tau", "La", "Ld")
    EPS = U32
    for v in range(n_vec):
        adj = {k: t.cpu().numpy().astype(np.float64) for k, t in
               sensor.band_radiance_srf_vjp(grid, t_d, a_d, d_d, Xk, E_d, Ts_s, s, cot[..., v]).items()}
        G = {"tau": adj["G_tau"], "La": adj["G_La"], "Ld": adj["G_Ld"]}
        c64 = cot[:, :, v].astype(np.float64)
        lhs = float(np.sum(c64 * dL[:, :, v]))
        rhs = float(sum(np.sum(grad[w][:, v] * atm[w][:, v]) for w in WRT) + grad["Ts_surface"][v] * surf["Ts_surface"][v]
                    + np.sum(grad["emis"][..., v] * surf["emis"][..., v].astype(np.float64)))
        d_s = dict(d_tau=r32["tau"][:, v], d_La=r32["La"][:, v], d_Ld=r32["Ld"][:, v], d_Ts=surf["Ts_surface"][v:v + 1],
                   d_E=surf["emis"][..., v])
        _, sc = JC.tangent(X, tables, tau.astype(np.float32), La.astype(np.float32), Ld.astype(np.float32), Xk, E, [Ts_s], **d_s)
        o = VC.adjoint(X, tables, tau.astype(np.float32), La.astype(np.float32), Ld.astype(np.float32), Xk, E, [Ts_s], cot[None, ..., v])
        bound = 32 * EPS * float(np.sum(np.abs(c64) * sc[0]))
        for key, skey, k in (("d_tau", "G_tau", K_ROW["G_tau"]), ("d_La", "G_La", K_ROW["G_La"]), ("d_Ld", "G_Ld", K_ROW["G_Ld"]),
                             ("d_Ts", "dTs", K_DTS), ("d_E", "dE", K_DE)):
            bound += k * EPS * float(np.sum(o["scale"][skey] * np.abs(np.asarray(d_s[key]).astype(np.float64))))
        v_sum = sum(np.abs(atm[w][:, v]).sum() for w in WRT)
        for i_, name in enumerate(names):
            S_J, want = 0.0, 0.0
            for w in WRT:
                Jw = np.abs(J[w][i_])
                den = np.maximum(np.maximum(Jw, 1e-3 * np.max(Jw, axis=0, keepdims=True)), F32_FLOOR)
                S_J = S_J + den @ np.abs(atm[w][:, v])
                want = want + J[w][i_] @ atm[w][:, v]
            bound += float(np.sum(np.abs(G[name]) * (2.0 * TOL_L * S_J + F32_TINY * v_sum + U32 * np.abs(want))))
        g_sum = sum(np.abs(G[name]).sum() for name in names)
        for w in WRT:
            scale_w = sum(np.abs(G[name]) @ np.abs(J[w][i_]) for i_, name in enumerate(names))  # [nL]
            bound += float(np.sum(np.abs(atm[w][:, v]) * (4.0 * U32 * scale_w + F32_TINY * g_sum)))
        print("band adjoint identity, vector %d: %.9g vs %.9g, |diff| = %.3g, bound %.3g" % (v, lhs, rhs, abs(lhs - rhs), bound))
        assert lhs != 0.0 and abs(lhs - rhs) <= bound
    # the continuum is in the gradient: the plain call's differs
    _, _, plain = rt.compute_band_radiance_vjp(XMIN, XMAX, s, Xk, E, Ts_s, cot, wrt=WRT, line_table=e["tbl"], dT_method="analytic",
                                               **dict(e["a"], Altitudes=np.array([500.0])))
    assert not np.allclose(plain[1], grad[1], rtol=1e-2, atol=0.0)


def test_fd_and_analytic_routes_agree(mods, e2e):
    """tests/test_gpu_jacobian_dT.py::test_band_radiance_vjp_matches_the_fd_route under continuum_derivatives=True: everything
    but the "T" entry has the "fd" route's bits; the "T" entries differ by at most TOL_T sum|g J|."""
    rt, eng, sensor, e = mods["rt"], mods["engine"], mods["sensor"], e2e
    s, Xk, E, Ts_s, rng = _band_case(mods, e)
    kw = _kw(e, Altitudes=np.array([500.0]))
    cot = rng.normal(size=(3, 3)).astype(np.float32)
    _, L_an, g_an = rt.compute_band_radiance_vjp(XMIN, XMAX, s, Xk, E, Ts_s, cot, wrt=WRT, dT_method="analytic", **kw)
    _, L_fd, g_fd = rt.compute_band_radiance_vjp(XMIN, XMAX, s, Xk, E, Ts_s, cot, wrt=WRT, **kw)
    assert np.array_equal(L_an, L_fd)
    for k in (1, 2, "Ts_surface", "emis"):
        assert np.array_equal(g_an[k], g_fd[k]), k
    X, tau, La, Ld = rt.compute_TUD(XMIN, XMAX, line_table=e["tbl"], continuum=e["cont"], **dict(e["a"], Altitudes=np.array([500.0])))
    grid = eng.Grid(XMIN, XMAX, X.size)
    dev32 = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float32).ravel(), device="cuda")
    rows = sensor.band_radiance_srf_vjp(grid, dev32(tau), dev32(La), dev32(Ld), Xk, torch.as_tensor(E, device="cuda"), Ts_s, s, cot)
    G = {k: rows[k].double().cpu().numpy() for k in ("G_tau", "G_La", "G_Ld")}
    _, _, _, _, J = rt.compute_TUD_jacobian(XMIN, XMAX, wrt=("T",), dT_method="analytic", **kw)
    dtau, dLa, dLd = J["T"]  # [nX][nL] each (one altitude)
    scale = np.abs(G["G_tau"]) @ np.abs(dtau) + np.abs(G["G_La"]) @ np.abs(dLa) + np.abs(G["G_Ld"]) @ np.abs(dLd)
    err = np.abs(g_an["T"] - g_fd["T"])
    print("band radiance vjp, T: worst |analytic - fd| / sum|g J| = %.3e (bound %.0e)" % (float(np.max(err / np.maximum(scale, 1e-300))), TOL_T))
    assert np.count_nonzero(g_an["T"]) >= 2 and np.all(np.isfinite(g_an["T"])) and not np.array_equal(g_an["T"], g_fd["T"])
    assert np.all(err <= TOL_T * scale)


def test_without_a_continuum_the_option_changes_no_bit(mods, e2e):
    rt, e = mods["rt"], e2e
    s, Xk, E, Ts_s, rng = _band_case(mods, e)
    kw = dict(line_table=e["tbl"], **e["a"])
    one = dict(kw, Altitudes=np.array([500.0]))
    cot = rng.normal(size=(3, 3)).astype(np.float32)
    g = {"tau": rng.normal(size=(e["X"].size, ALTS.size))}
    tang = {"T": rng.normal(size=e["nL"]), 2: rng.normal(size=e["nL"])}
    calls = [lambda **k: rt.compute_TUD_jacobian(XMIN, XMAX, wrt=WRT, **dict(kw, **k)),
             lambda **k: rt.compute_TUD_vjp(XMIN, XMAX, g, wrt=WRT, dT_method="analytic", **dict(kw, **k)),
             lambda **k: rt.compute_TUD_jvp(XMIN, XMAX, tang, **dict(kw, **k)),
             lambda **k: rt.compute_band_radiance_vjp(XMIN, XMAX, s, Xk, E, Ts_s, cot, wrt=WRT, **dict(one, **k)),
             lambda **k: rt.compute_band_radiance_jvp(XMIN, XMAX, s, Xk, E, Ts_s, dict(tang, Ts_surface=0.3), **dict(one, **k))]

    def leaves(r):
        if isinstance(r, dict):
            return [x for k in sorted(r, key=str) for x in leaves(r[k])]
        if isinstance(r, (tuple, list)):
            return [x for v in r for x in leaves(v)]
        return [np.asarray(r)]
    for fn in calls:
        a, b, c = leaves(fn()), leaves(fn(continuum_derivatives=True)), leaves(fn(continuum=None, continuum_derivatives=True))
        assert len(a) == len(b) == len(c) and len(a) >= 3
        for x, y, z in zip(a, b, c):
            assert np.array_equal(x, y, equal_nan=True) and np.array_equal(x, z, equal_nan=True)


def test_the_default_still_refuses(mods, e2e):
    rt, e = mods["rt"], e2e
    kw = dict(line_table=e["tbl"], continuum=e["cont"], **e["a"])
    calls = [(rt.compute_TUD_jacobian, ()), (rt.compute_TUD_vjp, ({"tau": np.ones((e["X"].size, ALTS.size))},)),
             (rt.compute_TUD_jvp, ({"T": np.ones(4)},)), (rt.compute_band_radiance_vjp, (None, None, None, 296.0, None)),
             (rt.compute_band_radiance_jvp, (None, None, None, 296.0, None))]
    for fn, rest in calls:
        for more in (dict(), dict(continuum_derivatives=False)):
            with pytest.raises(NotImplementedError, match=fn.__name__ + ": continuum is not supported"):
                fn(XMIN, XMAX, *rest, **dict(kw, **more))
    # what stays refused with the option on
    on = dict(kw, continuum_derivatives=True)
    with pytest.raises(NotImplementedError, match="broadening"):
        rt.compute_TUD_jacobian(XMIN, XMAX, broadening="self", **on)
    with pytest.raises(NotImplementedError, match="theta_r"):
        rt.compute_TUD_jacobian(XMIN, XMAX, **dict(on, theta_r=np.array([0.0, 0.3])))
    c9 = K.component(mods["ct"], 9, 950.0, 10.0, 12, seed=6)
    with pytest.raises(ValueError, match=r"molecule\(s\) \[9\]"):
        rt.compute_TUD_jacobian(XMIN, XMAX, **dict(on, continuum=c9))
