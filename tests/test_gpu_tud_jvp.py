"""rtx_tud_jvp (engine.tud_jvp_from_od, rt.compute_TUD_jvp): the tangent-linear TUD, J v without J, on the synthetic float32
columns of tests/tud_vjp_cases.py with the tangents of tests/tud_jvp_cases.py.

a. against the fp64 oracle (cpu_ref.jacobian_from_od over all layers, contracted with v on the host), on the flagged
   cases: |got - ref| <= TOL_L S + 2^-24 |ref|, S = sum_{w,l} |v| max(|J_oracle|, 1e-3 rowmax, 1e-30): the element-wise
   bound of tests/test_gpu_tud_paths.py weighted by |v|, plus the one float32 rounding of the output. It is what a
   contraction of a stored J that passes that test file would be allowed. Two of them again with two layer altitudes
   exchanged (a tau mask that is not a run of the lowest layers: the kernel's masked sweep).
b. the two unflagged cases, where the stored J itself misses TOL_L: the same with TOL_L max(1, r_J), r_J the worst ratio of
   the stored Jacobian's own error to its bound on the same inputs (the parent's kernel, not the code under test).
c. row groups, d. structural zeros, e. N_angle = 1, f. bit identity, g. the adjoint identity <G, J v> = <J^T G, v> against
   rtx_tud_vjp, h. rt.compute_TUD_jvp end to end, i. the results are, bit for bit, what the parent commit's build
   gave.

Measured (MI355X; worst ratio of the error to the bound over all elements): a. 0.003, 0.019, 0.017, 0.021,
0.047 (cases 0-4), 0.021 and 0.047 with unsorted layer altitudes (cases 3, 4); b. r_J = 9.58 and 9.04, the tangent's own ratio at TOL_L 0.094 and 0.073 (0.0098 and 0.0081 of the
asserted bound); g. 8.5e-5 to 1.6e-3; h. 3.1e-12 (tau, an opaque window), 0.0075 (La), 0.017 (Ld)."""
import hashlib

import numpy as np
import pytest

import tud_jvp_cases as cases
from oracle import cpu_ref as ref
from radtxfr_amd import synthetic

pytestmark = pytest.mark.gpu

TOL_L = 1e-5         # tests/test_gpu_tud_paths.py
U32 = 2.0 ** -24
F32_TINY = 2.0 ** -126  # the smallest normal float32
H_T = cases.H_T
SENTINEL = -7.25


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib, engine
    _lib.load()
    return engine


def _grid(eng, n, lo=700.0):
    return eng.Grid(lo, lo + 1.5, n) if n > 1 else eng.Grid(lo, lo + 1.5, 64).shard(37, 1)  # a one-point shard


def _dev(a, pad=0):
    """float32 on the device with a padded leading dimension, the padding NaN: it must not leak."""
    import torch
    a = np.asarray(a, dtype=np.float32)
    n = a.shape[-1]
    b = np.full(a.shape[:-1] + (n + pad,), np.nan, dtype=np.float32)
    b[..., :n] = a
    return torch.as_tensor(b, device="cuda")[..., :n]


def _rows(d, nZ):
    """{name: tensor} -> float64 NumPy [n_vec][2 nZ + 1][n] (all three groups present)."""
    return np.concatenate([d["tau"].double().cpu().numpy(), d["La"].double().cpu().numpy(),
                           d["Ld"].double().cpu().numpy()[:, None, :]], axis=1)


class Run:
    """One configuration on the device: its columns, its tangents, the reference and the product of all three row groups."""

    def __init__(self, eng, case, c=None):
        c = self.c = cases.make(case) if c is None else c
        self.eng = eng
        self.grid = _grid(eng, c["n"])
        pad = c["pad"]
        self.cols = dict(OD=_dev(c["OD"], pad), ODp=_dev(c["ODp"], pad) if c["with_T"] else None,
                         ODm=_dev(c["ODm"], pad) if c["with_T"] else None, K=_dev(c["K"], pad) if c["n_spec"] else None,
                         tau=None if c["returnOD"] else _dev(c["tau32"], pad))
        self.nZ = c["alts"].size
        self.V = cases.tangents(c)
        self.ref, self.S, self.dense = cases.reference(c, self.grid.axis(), ref, self.V)
        self.out = self.jvp(self.V)
        self.got = _rows(self.out, self.nZ)

    def kw(self, layers=None, N_angle=None):
        c = self.c
        return dict(Altitudes=c["alts"], theta_r=c["theta"], N_angle=c["nA"] if N_angle is None else N_angle,
                    returnOD=c["returnOD"], layers=c["layers"] if layers is None else layers, t_pos=c["t_pos"])

    def jvp(self, V, rows=("tau", "La", "Ld"), layers=None, tau="given", N_angle=None, grid=None, cols=None, dOD_dT=None):
        k = self.cols if cols is None else cols
        fd = (k["ODp"], k["ODm"], H_T) if dOD_dT is None else (None, None, H_T)
        return self.eng.tud_jvp_from_od(k["OD"], fd[0], fd[1], fd[2], k["K"], k["tau"] if tau == "given" else None,
                                        self.grid if grid is None else grid, self.c["T"], self.c["Z"], V, rows=rows,
                                        dOD_dT=dOD_dT, **self.kw(layers, N_angle))

    def jacobian(self, layers=None):
        k = self.cols
        return self.eng.tud_jacobian_from_od(k["OD"], k["ODp"], k["ODm"], H_T, k["K"], k["tau"], self.grid, self.c["T"],
                                             self.c["Z"], **self.kw(layers))


_RUNS = {}


@pytest.fixture(scope="module")
def run(eng):
    def get(case):
        if case not in _RUNS:
            _RUNS[case] = Run(eng, case)
        return _RUNS[case]
    yield get
    _RUNS.clear()


def _within(got, want, bound, what):
    """|got - want| <= bound element by element; returns (and prints) the worst ratio to the bound."""
    err = np.abs(got - want)
    ok = err <= bound
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    print("%s: worst |got - ref| / bound = %.3g" % (what, ratio))
    assert ok.all(), (what, ratio, np.argwhere(~ok)[:5])
    return ratio


def _same_bits(a, b):
    return all(np.array_equal(a[k].cpu().numpy().view(np.uint32), b[k].cpu().numpy().view(np.uint32)) for k in a) and set(a) == set(b)


ALL = range(len(cases.CASES))
FLAGGED = [i for i in ALL if cases.CASES[i][-1]]


def _shapes(r):
    c = r.c
    assert r.out["tau"].shape == r.out["La"].shape == (c["n_vec"], r.nZ, c["n"]) and r.out["Ld"].shape == (c["n_vec"], c["n"])
    assert all(t.dtype.is_floating_point and t.element_size() == 4 for t in r.out.values())
    assert np.isfinite(r.got).all() and np.isfinite(r.ref).all()
    assert np.count_nonzero(r.ref) > 0.3 * r.ref.size


# ------------------------------------------------------------------------------------------------ a. the fp64 oracle
@pytest.mark.parametrize("case", FLAGGED)
def test_jvp_vs_fp64_oracle(run, case):
    r = run(case)
    _shapes(r)
    _within(r.got, r.ref, TOL_L * r.S + U32 * np.abs(r.ref), "case %d vs oracle" % case)


@pytest.mark.parametrize("case", [3, 4])
def test_jvp_vs_fp64_oracle_unsorted_layer_altitudes(eng, case):
    """Two layer altitudes exchanged: the Z <= zs mask of an altitude between them is no longer its first count layers, so
    its tau row sums a masked set of layers while its L-up row still takes the first count (the reference's quirk). Same
    columns, same bound as (a)."""
    c = cases.make(case)
    Z = c["Z"].copy()
    Z[1], Z[-2] = Z[-2], Z[1]
    masks = [Z <= zs for zs in c["alts"]]
    assert any(m.sum() and not m[:int(m.sum())].all() for m in masks)
    with np.errstate(over="ignore"):
        tau32 = np.stack([np.exp(-c["mu"] * c["OD"].astype(np.float64)[m].sum(axis=0)) for m in masks]).astype(np.float32)
    r = Run(eng, case, dict(c, Z=Z, tau32=tau32))
    _shapes(r)
    _within(r.got, r.ref, TOL_L * r.S + U32 * np.abs(r.ref), "case %d, unsorted Z, vs oracle" % case)
    for rows in (("tau",), ("tau", "Ld")):
        assert _same_bits(r.jvp(r.V, rows=rows), {k: r.out[k] for k in rows}), rows


# ------------------------------------------------------------------------------------------------ b. the unflagged cases
@pytest.mark.parametrize("case", [i for i in ALL if i not in FLAGGED])
def test_jvp_vs_fp64_oracle_where_the_stored_jacobian_misses(run, case):
    r = run(case)
    _shapes(r)
    c = r.c
    Jo, den = cases.oracle_all_layers(c, r.grid.axis(), ref)
    J = r.jacobian(layers=list(range(c["nL"]))).double().cpu().numpy()
    r_J = float(np.max(np.abs(J - Jo) / (TOL_L * den)))
    print("case %d: stored J vs oracle, worst error / bound r_J = %.3g" % (case, r_J))
    own = float(np.max(np.abs(r.got - r.ref) / np.maximum(TOL_L * r.S + U32 * np.abs(r.ref), 1e-300)))
    print("case %d: the tangent's own ratio at TOL_L = %.3g" % (case, own))
    _within(r.got, r.ref, TOL_L * max(1.0, r_J) * r.S + U32 * np.abs(r.ref), "case %d vs oracle, TOL_L max(1, r_J)" % case)


# ------------------------------------------------------------------------------------------------ c. row groups
@pytest.mark.parametrize("case", [1, 5, 6])
def test_row_groups(eng, run, case):
    import torch
    r = run(case)
    for rows in (("tau",), ("La",), ("Ld",), ("La", "Ld"), ("tau", "Ld"), ("tau", "La")):
        got = r.jvp(r.V, rows=rows, tau="given" if "tau" in rows else None)  # tau=None is fine without "tau"
        assert set(got) == set(rows)
        assert _same_bits(got, {k: r.out[k] for k in rows}), rows
    # a group that is not requested is not written: the library call itself, on sentinel-filled arrays
    c = r.c
    lib = eng._lib.load()
    f = eng._jacobian_front("tud_jvp", lib.rtx_tud_jvp, lib.rtx_tud_jvp_dod, r.cols["OD"], r.cols["ODp"], r.cols["ODm"], H_T,
                            r.cols["K"], r.cols["tau"], r.grid, c["T"], c["Z"], c["alts"], c["theta"], c["nA"], c["returnOD"],
                            None, None)
    n, nv = c["n"], min(c["n_vec"], lib.rtx_tud_jvp_max_vectors())
    dense = np.ascontiguousarray(r.dense[:nv])
    for keep in ((True, False, False), (False, True, False), (False, False, True)):
        bufs = [torch.full((nv, r.nZ, n + 3), SENTINEL, dtype=torch.float32, device="cuda") for _ in range(2)]
        bufs.append(torch.full((nv, n + 3), SENTINEL, dtype=torch.float32, device="cuda"))
        # every array is handed over only when kept; the others must stay as they are, and so must the padding
        ptrs = [eng._ptr(b) if k else None for b, k in zip(bufs, keep)]
        eng._lib.check(f.entry(*f.lead, c["t_pos"], dense.ctypes.data, nv, ptrs[0], ptrs[1], ptrs[2], n + 3,
                               eng._stream_ptr()))
        torch.cuda.synchronize()
        for b, k, name in zip(bufs, keep, ("tau", "La", "Ld")):
            h = b.cpu().numpy()
            assert np.all(h[..., n:] == SENTINEL), name
            if k:
                assert np.array_equal(h[..., :n].view(np.uint32), r.out[name][:nv].cpu().numpy().view(np.uint32)), name
            else:
                assert np.all(h == SENTINEL), name


# ------------------------------------------------------------------------------------------------ d. exact zeros
@pytest.mark.parametrize("case", [4, 5, 6])
def test_structural_zeros_are_exact(run, case):
    r = run(case)
    c = r.c
    nZ, nL = r.nZ, c["nL"]
    # the all-zero vector (vector 1 of every case with more than one)
    assert not r.V[1].any() and np.all(r.got[1] == 0.0)
    assert np.count_nonzero(r.got[0]) > 0.3 * r.got[0].size
    # an altitude below the surface: no layer in its mask, count 0 -- its tau and L-up rows are exact zeros, as J's are
    counts = [int((c["Z"] <= zs).sum()) for zs in c["alts"]]
    below = [a_ for a_, cnt in enumerate(counts) if cnt == 0]
    assert below
    for a_ in below:
        assert np.all(r.got[:, a_] == 0.0) and np.all(r.got[:, nZ + a_] == 0.0)
    # L-up of an altitude inside the column: layers at or above its count contribute exactly nothing
    a_ = int(np.argmin([cnt if cnt > 0 else 10 ** 6 for cnt in counts]))
    assert 0 < counts[a_] < nL and 0 < counts[-1] < nL
    layers = list(range(nL))
    rng = np.random.default_rng(case)
    V = rng.normal(size=(2, len(c["wrt"]), nL))
    base = r.jvp(V, layers=layers)
    for name, cnt, pick in (("La", counts[a_], a_), ("Ld", counts[-1], None)):
        W = V.copy()
        W[:, :, cnt:] = rng.normal(size=W[:, :, cnt:].shape) * 50.0
        moved = r.jvp(W, layers=layers)
        b, m = base[name].cpu().numpy(), moved[name].cpu().numpy()
        if pick is not None:
            b, m = b[:, pick], m[:, pick]
        assert np.array_equal(b.view(np.uint32), m.view(np.uint32)), name
        assert np.count_nonzero(b) > 0.3 * b.size
        # and a vector that lives there alone gives exact zeros
        W[:, :, :cnt] = 0.0
        z = r.jvp(W, layers=layers)[name].cpu().numpy()
        assert np.all((z if pick is None else z[:, pick]) == 0.0), name
    assert not _same_bits(base, moved)  # (the rows that do see those layers moved)


# ------------------------------------------------------------------------------------------------ e. N_angle = 1
def test_single_angle(run):
    r = run(6)
    one = r.jvp(r.V, N_angle=1)
    two = r.jvp(r.V, N_angle=2)
    assert np.isnan(one["Ld"].cpu().numpy()).all()
    assert np.isfinite(two["Ld"].cpu().numpy()).all()
    for name in ("tau", "La"):
        a, b = one[name].cpu().numpy(), two[name].cpu().numpy()
        assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    assert _same_bits(r.jvp(r.V, rows=("tau", "La"), N_angle=1), {k: r.out[k] for k in ("tau", "La")})


# ------------------------------------------------------------------------------------------------ f. bit identity
@pytest.mark.parametrize("case", [2, 5])
def test_bit_identity(eng, run, case, monkeypatch):
    r = run(case)
    c = r.c
    assert _same_bits(r.jvp(r.V), r.out)
    # a vector alone and among others, across the group boundary; every blocking of the vectors by the engine
    n_max = eng._lib.load().rtx_tud_jvp_max_vectors()
    assert c["n_vec"] == n_max + 1
    for v in range(c["n_vec"]):
        alone = r.jvp(r.V[v:v + 1])
        assert _same_bits(alone, {k: t[v:v + 1] for k, t in r.out.items()}), v
    for group in (1, 2, 3):
        monkeypatch.setattr(eng, "JVP_VEC_GROUP", group)
        assert _same_bits(r.jvp(r.V), r.out), group
    monkeypatch.setattr(eng, "JVP_VEC_GROUP", None)
    # a single vector given without the vector axis
    assert _same_bits(r.jvp(r.V[0]), {k: t[0:1] for k, t in r.out.items()})
    # layers permuted together with V
    rng = np.random.default_rng(case)
    perm = rng.permutation(len(c["layers"]))
    assert _same_bits(r.jvp(r.V[:, :, perm], layers=[c["layers"][p] for p in perm]), r.out)
    # a shard that does not start on a multiple of 4 equals the slice of the full call
    n = c["n"]
    h, m = 5, n - 7
    assert h % 4 != 0 and m > 0
    cols = {k: (None if t is None else t[..., h:h + m]) for k, t in r.cols.items()}
    part = r.jvp(r.V, grid=r.grid.shard(h, m), cols=cols)
    assert _same_bits(part, {k: t[..., h:h + m] for k, t in r.out.items()})


@pytest.mark.parametrize("case", [1, 5])
def test_dod_entry_equals_the_fd_entry(run, case):
    """(ODp - ODm) / (2 H_T) is exact in float32 for these inputs (tud_vjp_cases.make), so the derivative given directly is
    the number the fd entry forms."""
    r = run(case)
    c = r.c
    assert c["with_T"]
    d32 = (c["ODp"] - c["ODm"]) / np.float32(2.0 * H_T)
    assert d32.dtype == np.float32
    assert np.array_equal(d32.astype(np.float64), (c["ODp"].astype(np.float64) - c["ODm"].astype(np.float64)) / (2.0 * H_T))
    assert _same_bits(r.jvp(r.V, dOD_dT=_dev(d32, c["pad"])), r.out)


# ------------------------------------------------------------------------------------------------ g. the adjoint identity
@pytest.mark.parametrize("case", FLAGGED)
def test_adjoint_identity(run, case):
    """<G, J v> from rtx_tud_jvp against <J^T G, v> from rtx_tud_vjp, per vector, both sums in fp64 on the host:
    |lhs - rhs| <= sum|G| (bound of a) + sum|v| (bound b of tests/test_gpu_tud_vjp.py), the two sides' own bounds."""
    r = run(case)
    c = r.c
    nZ = r.nZ
    k = r.cols
    G32 = np.asarray(c["G"], dtype=np.float32)
    G = G32.astype(np.float64)
    grad = r.eng.tud_vjp_from_od(k["OD"], k["ODp"], k["ODm"], H_T, k["K"], k["tau"], r.grid, c["T"], c["Z"], G_tau=G32[:, :nZ],
                                 G_Lu=G32[:, nZ:2 * nZ], G_Ld=G32[:, 2 * nZ], **r.kw()).cpu().numpy()
    lhs = np.einsum("vrn,vrn->v", G, r.got)
    rhs = np.einsum("vwk,vwk->v", grad, r.V)
    bound_a = TOL_L * r.S + U32 * np.abs(r.ref)
    # bound b of the adjoint's test: TOL_L sum|G| den + 4 2^-24 sum|G J_stored|, on the case's layers list
    Jo = cases.oracle_jacobian(c, r.grid.axis(), ref)
    rowmax = np.max(np.abs(Jo), axis=-1, keepdims=True)
    den = np.maximum(np.maximum(np.abs(Jo), 1e-3 * rowmax), cases.F32_FLOOR)
    J = r.jacobian().double().cpu().numpy()
    bound_b = TOL_L * np.einsum("vrn,wkrn->vwk", np.abs(G), den) + 4.0 * U32 * np.einsum("vrn,wkrn->vwk", np.abs(G), np.abs(J))
    bound = np.einsum("vrn,vrn->v", np.abs(G), bound_a) + np.einsum("vwk,vwk->v", np.abs(r.V), bound_b)
    assert np.count_nonzero(lhs) >= max(1, c["n_vec"] - 1)
    _within(lhs, rhs, bound, "case %d adjoint identity" % case)


# ------------------------------------------------------------------------------------------------ h. end to end
def test_compute_tud_jvp_end_to_end(eng):
    import torch
    assert torch.cuda.is_available()
    from radtxfr_amd import radiative_transfer as rt
    lo, hi, dv = 1000.0, 1000.5, 0.0005
    full = synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
    sub = synthetic.subset_table(full, lo - 12.0, hi + 12.0)
    sa = rt.StdAtmos
    a = dict(Zs=sa[:, 1], Ts=sa[:, 5].copy(), Ps=sa[:, 4], PLs=sa[:, 3], MFs_VAL=sa[:, 6:9] * 1e6, MFs_ID=np.array([1, 2, 3]))
    alts = np.array([0.5, 30.0, 8.0])
    wrt = ("T", 1, 3)
    kw = dict(DVOUT=dv, line_table=sub, Altitudes=alts, **a)
    X, tau, La, Ld = rt.compute_TUD(lo, hi, **kw)
    nX, nL, nZ = X.size, a["Ts"].size, alts.size
    assert nL == 66
    rng = np.random.default_rng(4)
    n_vec = 2
    tang = {"T": rng.normal(size=(nL, n_vec)), 1: rng.normal(size=(nL, n_vec)) * 30.0, 3: rng.normal(size=(nL, n_vec)) * 0.1}
    tang["T"][10:20, 0] = 0.0
    Xv, tau_v, La_v, Ld_v, d = rt.compute_TUD_jvp(lo, hi, tang, **kw)
    assert np.array_equal(Xv, X) and np.array_equal(tau_v, tau) and np.array_equal(La_v, La) and np.array_equal(Ld_v, Ld)
    assert set(d) == {"tau", "La", "Ld"}
    assert d["tau"].shape == d["La"].shape == (nX, nZ, n_vec) and d["Ld"].shape == (nX, n_vec)
    assert all(v.dtype == np.float64 for v in d.values())
    Xj, _, _, _, J = rt.compute_TUD_jacobian(lo, hi, wrt=wrt, **kw)
    for i_, name in enumerate(("tau", "La", "Ld")):
        sub_x = "xal,lv->xav" if name != "Ld" else "xl,lv->xv"
        want = sum(np.einsum(sub_x, J[w][i_], tang[w]) for w in wrt)
        S_J = 0.0
        for w in wrt:
            Jw = np.abs(J[w][i_])
            den = np.maximum(np.maximum(Jw, 1e-3 * np.max(Jw, axis=0, keepdims=True)), cases.F32_FLOOR)
            S_J = S_J + np.einsum(sub_x, den, np.abs(tang[w]))
        v_sum = sum(np.abs(tang[w]).sum(axis=0) for w in wrt)  # [n_vec]
        if name != "tau":  # (this window is opaque: tau, and with it the stored J's tau rows, underflows float32 almost everywhere)
            assert np.count_nonzero(want) > 0.5 * want.size
        _within(d[name], want, 2.0 * TOL_L * S_J + F32_TINY * v_sum + U32 * np.abs(want), "end to end, %s" % name)
    # a trailing vector axis gives the stacked single-vector results; rows= restricts the dict, the bits stay
    for v in range(n_vec):
        one = rt.compute_TUD_jvp(lo, hi, {w: t[:, v] for w, t in tang.items()}, rows=("tau", "La"), **kw)[4]
        assert set(one) == {"tau", "La"}
        for name in one:
            assert one[name].shape == (nX, nZ) and np.array_equal(one[name], d[name][..., v]), (name, v)
    # layers=: the layers named move, the others do not
    lay = [65, 3, 8]
    some = rt.compute_TUD_jvp(lo, hi, {w: t[lay, 0] for w, t in tang.items()}, layers=lay, **kw)[4]
    z = {w: np.zeros(nL) for w in wrt}
    for w in wrt:
        z[w][lay] = tang[w][lay, 0]
    dense = rt.compute_TUD_jvp(lo, hi, z, **kw)[4]
    for name in dense:
        assert np.array_equal(some[name], dense[name]), name
    # dT_method="analytic" is engine.tud_jvp_from_od on engine.voigt_sum_dT's derivative, bit for bit
    d_an = rt.compute_TUD_jvp(lo, hi, tang, dT_method="analytic", **kw)[4]
    c = rt._Call("compute_TUD_jvp", lo, hi, rt.options, kw)
    s = eng._jacobian_stages("tud_jvp", c.table(), c.grid, c.Z, c.T, c.P, c.PL, c.MF, c.ID, c.Z_s, c.theta, c.N_angle, c.returnOD,
                             wrt, None, 0.5, None, "analytic")
    assert s.dOD_dT is not None and s.OD_plus is None
    dOD = torch.empty_like(s.dOD_dT)
    w_, p_atm = eng.layer_weights_od(c.table().species, c.T, c.P, c.PL, c.MF.reshape(nL, -1), c.ID)
    eng.voigt_sum_dT(c.table(), c.grid, s.T, p_atm, w_, dOD)
    assert torch.equal(dOD, s.dOD_dT)
    V = np.stack([tang[w].T for w in wrt], axis=1)  # [n_vec][n_wrt][nL]
    direct = eng.tud_jvp_from_od(s.OD, None, None, 0.5, s.K, s.tau, c.grid, s.T, s.Z, V, Altitudes=c.Z_s, theta_r=c.theta,
                                 N_angle=c.N_angle, returnOD=c.returnOD, t_pos=s.t_pos, dOD_dT=dOD)
    for name in ("tau", "La"):
        assert np.array_equal(d_an[name], direct[name].double().cpu().numpy().transpose(2, 1, 0)), name
    assert np.array_equal(d_an["Ld"], direct["Ld"].double().cpu().numpy().T)


# ------------------------------------------------------------------------------- i. the tangent kernel is untouched
# The seven non-empty selections of the row groups (tau, L-up, Ld): one instantiation of tud_jvp_kernel each.
SELECTIONS = [(t, u, d) for t in (False, True) for u in (False, True) for d in (False, True)][1:]

# SHA-256 over the concatenated bytes of the results (float32; tau [n_vec][n_alt][n], La the same, Ld [n_vec][n], those
# requested, in this order) that engine.tud_jvp_from_od gives for the seven SELECTIONS in that order, per case of cases.make
# with its tangents (cases.tangents); "dod": the same through rtx_tud_jvp_dod on case 1, the derivative given as
# (ODp - ODm) / (2 H_T). Recorded on an MI355X from a build of the parent commit 14c6c52 (before the entry glue of the
# three derivative files moved to rtx_tud_jac_common.h and the staged tangents to StreamScratch).
PARENT_JVP_SHA256 = {
    1: "9848f72d1d521f01fbe5875415115e2a97668e911756ffef096c5d970f2dcaf5",
    4: "ec36ec67bc51866443dc4d7d77ba7b5b168714803cea08f53738326aa8b6a7f2",
    6: "68b83a41b6ef4a9a42f13a01d20c0ca1f4c971f6e0aef27c31f8a70956a07d67",
    "dod": "9848f72d1d521f01fbe5875415115e2a97668e911756ffef096c5d970f2dcaf5",
}


def jvp_bits(r, dOD_dT=None):
    """The hash described above for a Run."""
    h = hashlib.sha256()
    for sel in SELECTIONS:
        rows = tuple(name for name, on in zip(("tau", "La", "Ld"), sel) if on)
        out = r.jvp(r.V, rows=rows, dOD_dT=dOD_dT)
        assert set(out) == set(rows)
        for name in rows:
            a = out[name].contiguous().cpu().numpy()
            assert a.dtype == np.float32 and a.shape == r.out[name].shape
            h.update(a.tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("case", [1, 4, 6])
def test_jvp_bits_are_the_parent_commits(run, case):
    assert jvp_bits(run(case)) == PARENT_JVP_SHA256[case]


def test_jvp_dod_bits_are_the_parent_commits(run):
    r = run(1)
    c = r.c
    d32 = (c["ODp"] - c["ODm"]) / np.float32(2.0 * H_T)  # exact in float32 for these inputs (tud_vjp_cases.make)
    assert d32.dtype == np.float32
    assert jvp_bits(r, dOD_dT=_dev(d32, c["pad"])) == PARENT_JVP_SHA256["dod"]
