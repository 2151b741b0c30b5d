"""rtx_tud_vjp (engine.tud_vjp_from_od, rt.compute_TUD_vjp): the adjoint of the TUD Jacobian, on the synthetic float32
columns of tests/test_gpu_tud_paths.py (tests/tud_vjp_cases.py).

a. against the stored Jacobian of the same inputs (engine.tud_jacobian_from_od) contracted in fp64 on the host:
   |got - ref| <= 4 2^-24 sum|G J| for every (vector, wrt, layer). A stored J element is the fp32 rounding (2^-24 relative)
   of a value the adjoint keeps in fp64; 4 is margin for the same fp32 row factors being combined in another order.
b. against the fp64 oracle (cpu_ref.jacobian_from_od on the same float32 inputs), on the configurations where the stored J
   itself is within TOL_L of it (asserted): TOL_L sum|G| max(|J_oracle|, 1e-3 rowmax, 1e-30) plus the term of (a) -- the
   element-wise bound of tests/test_gpu_tud_paths.py weighted by |G|.
   The end-to-end case (g) adds 2^-126 sum|G| to it: a J element below the smallest normal float32 (2^-126) is stored as
   a subnormal or as 0 and is then NOT a 2^-24-relative rounding of its value, which the adjoint still carries in fp64
   (the standard atmosphere's H2O sensitivities at 13-14 km in this window underflow float32: J holds 0 in every row, the
   adjoint a non-zero sum). The term is the stored reference's own error, 1e-38 per unit of |G|; the synthetic cases do
   not need it.
c. row groups left out, d. structural zeros, e. N_angle = 1, f. bit identity, g. rt.compute_TUD_vjp end to end,
h. the Jacobian kernel's own results are what they were before its helpers moved to a shared header,
i. the adjoint's own results are what the parent commit's build gave.

Measured (MI355X; worst ratio of the error to the bound over all elements): a. 0.12 (the one-point shard;
0.04-0.07 otherwise), b. 0.017, c. 0.09, g. 0.084."""
import hashlib

import numpy as np
import pytest

import tud_vjp_cases as cases
from oracle import cpu_ref as ref
from radtxfr_amd import synthetic

pytestmark = pytest.mark.gpu

TOL_L = 1e-5         # tests/test_gpu_tud_paths.py
F32_FLOOR = 1e-30
U32 = 2.0 ** -24
F32_TINY = 2.0 ** -126  # the smallest normal float32
H_T = cases.H_T


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


class Run:
    """One configuration on the device: its columns, the stored Jacobian and the adjoint of all three row groups."""

    def __init__(self, eng, case):
        c = self.c = cases.make(case)
        self.eng = eng
        self.grid = _grid(eng, c["n"])
        pad = c["pad"]
        self.cols = dict(OD=_dev(c["OD"], pad), ODp=_dev(c["ODp"], pad) if c["with_T"] else None,
                         ODm=_dev(c["ODm"], pad) if c["with_T"] else None, K=_dev(c["K"], pad) if c["n_spec"] else None,
                         tau=None if c["returnOD"] else _dev(c["tau32"], pad))
        nZ = self.nZ = c["alts"].size
        self.G = c["G"]
        self.J = self.jacobian().double().cpu().numpy()
        self.grad = self.vjp(self.G)

    def kw(self, layers=None):
        c = self.c
        return dict(Altitudes=c["alts"], theta_r=c["theta"], N_angle=c["nA"], returnOD=c["returnOD"],
                    layers=c["layers"] if layers is None else layers, t_pos=c["t_pos"])

    def jacobian(self, layers=None):
        k = self.cols
        return self.eng.tud_jacobian_from_od(k["OD"], k["ODp"], k["ODm"], H_T, k["K"], k["tau"], self.grid, self.c["T"], self.c["Z"],
                                             **self.kw(layers))

    def vjp(self, G, groups=(True, True, True), layers=None, tau="given", pad=None, N_angle=None):
        """G [n_vec][2 nZ + 1][n] (NumPy); groups: which of (tau, L-up, Ld) are passed at all."""
        k = self.cols
        nZ = self.nZ
        pad = self.c["pad"] if pad is None else pad
        G = np.asarray(G, dtype=np.float32)
        kw = self.kw(layers)
        if N_angle is not None:
            kw["N_angle"] = N_angle
        out = self.eng.tud_vjp_from_od(k["OD"], k["ODp"], k["ODm"], H_T, k["K"], k["tau"] if tau == "given" else None, self.grid,
                                       self.c["T"], self.c["Z"], G_tau=_dev(G[:, :nZ], pad) if groups[0] else None,
                                       G_Lu=_dev(G[:, nZ:2 * nZ], pad) if groups[1] else None,
                                       G_Ld=_dev(G[:, 2 * nZ], pad) if groups[2] else None, **kw)
        assert out.dtype.is_floating_point and out.element_size() == 8
        return out.cpu().numpy()


_RUNS = {}


@pytest.fixture(scope="module")
def run(eng):
    def get(case):
        if case not in _RUNS:
            _RUNS[case] = Run(eng, case)
        return _RUNS[case]
    yield get
    _RUNS.clear()


def _within(got, want, scale, what, factor=4.0 * U32, extra=0.0, g_sum=0.0):
    """|got - want| <= factor scale + extra + F32_TINY g_sum, element by element; returns the worst ratio to the bound.
    g_sum = sum|G| over the contracted elements, for references built from a float32-stored J (see the module docstring)."""
    bound = factor * scale + extra + F32_TINY * g_sum
    err = np.abs(got - want)
    ok = err <= bound
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    print("%s: worst |got - ref| / bound = %.3g" % (what, ratio))
    assert ok.all(), (what, ratio, np.argwhere(~ok)[:5])
    return ratio


ALL = range(len(cases.CASES))


# ------------------------------------------------------------------------------------------------ a. the stored Jacobian
@pytest.mark.parametrize("case", ALL)
def test_vjp_vs_contracted_stored_jacobian(run, case):
    r = run(case)
    c = r.c
    assert r.grad.shape == (c["n_vec"], len(c["wrt"]), len(c["layers"])) and r.grad.dtype == np.float64
    assert np.isfinite(r.grad).all() and np.isfinite(r.J).all()
    want, scale = cases.contract(r.G, r.J)
    assert np.count_nonzero(want) > 0.5 * want.size
    _within(r.grad, want, scale, "case %d vs stored J" % case)


# ------------------------------------------------------------------------------------------------ b. the fp64 oracle
@pytest.mark.parametrize("case", [i for i in ALL if cases.CASES[i][-1]])
def test_vjp_vs_fp64_oracle(run, case):
    r = run(case)
    c = r.c
    Jo = cases.oracle_jacobian(c, r.grid.axis(), ref)
    rowmax = np.max(np.abs(Jo), axis=-1, keepdims=True)
    den = np.maximum(np.maximum(np.abs(Jo), 1e-3 * rowmax), F32_FLOOR)
    # the premise: the stored Jacobian of this configuration meets TOL_L, row by row (the _rel measure)
    worst_J = float(np.max(np.abs(r.J - Jo) / den))
    print("case %d: stored J vs oracle, worst rel_err %.3g" % (case, worst_J))
    assert worst_J <= TOL_L, (case, worst_J)
    want, _ = cases.contract(r.G, Jo)
    _, scale_a = cases.contract(r.G, r.J)
    bound_b = TOL_L * np.einsum("vrn,wkrn->vwk", np.abs(r.G.astype(np.float64)), den)
    _within(r.grad, want, bound_b, "case %d vs oracle" % case, factor=1.0, extra=4.0 * U32 * scale_a)


# ------------------------------------------------------------------------------------------------ c. row groups
@pytest.mark.parametrize("case", [1, 5, 6])
def test_row_groups_alone(run, case):
    r = run(case)
    nZ = r.nZ
    sl = {0: slice(0, nZ), 1: slice(nZ, 2 * nZ), 2: slice(2 * nZ, 2 * nZ + 1)}
    for gi, name in enumerate(("tau", "Lu", "Ld")):
        groups = tuple(i == gi for i in range(3))
        Gz = np.zeros_like(r.G)
        Gz[:, sl[gi]] = r.G[:, sl[gi]]
        alone = r.vjp(r.G, groups=groups, tau="given" if gi == 0 else None)  # tau=None is fine without G_tau
        padded = r.vjp(Gz)
        want, scale = cases.contract(r.G[:, sl[gi]], r.J[:, :, sl[gi]])
        _within(alone, want, scale, "case %d %s alone vs stored J" % (case, name))
        _within(alone, padded, scale, "case %d %s alone vs zero-padded" % (case, name))


def test_two_groups_and_no_tau(run):
    r = run(6)
    nZ = r.nZ
    got = r.vjp(r.G, groups=(False, True, True), tau=None)
    want, scale = cases.contract(r.G[:, nZ:], r.J[:, :, nZ:])
    _within(got, want, scale, "Lu + Ld without tau")
    got = r.vjp(r.G, groups=(True, False, True))
    keep = np.r_[0:nZ, 2 * nZ]
    want, scale = cases.contract(r.G[:, keep], r.J[:, :, keep])
    _within(got, want, scale, "tau + Ld")
    got = r.vjp(r.G, groups=(True, True, False))
    want, scale = cases.contract(r.G[:, :2 * nZ], r.J[:, :, :2 * nZ])
    _within(got, want, scale, "tau + Lu")


# ------------------------------------------------------------------------------------------------ d. exact zeros
@pytest.mark.parametrize("case", [4, 6])
def test_structural_zeros_are_exact(eng, run, case):
    r = run(case)
    c = r.c
    nZ = r.nZ
    layers = np.asarray(c["layers"])
    counts = [int((c["Z"] <= zs).sum()) for zs in c["alts"]]
    a_ = int(np.argmin([cnt if cnt > 0 else 10 ** 6 for cnt in counts]))  # the lowest altitude inside the column
    assert 0 < counts[a_] < c["nL"] and 0 < counts[-1] < c["nL"]
    G = np.zeros_like(r.G)
    G[:, nZ + a_] = 1.0 + np.abs(r.G[:, 2 * nZ])
    for groups in ((True, True, True), (False, True, False)):
        got = r.vjp(G, groups=groups)
        above = layers >= counts[a_]
        assert above.any() and (~above).any()
        assert np.all(got[:, :, above] == 0.0), (case, groups)
        assert np.count_nonzero(got[:, :, ~above]) > 0  # (a layer of zero optical depth below the count gives 0 too)
    G = np.zeros_like(r.G)
    G[:, 2 * nZ] = 1.0 + np.abs(r.G[:, 0])
    for groups in ((True, True, True), (False, False, True)):
        got = r.vjp(G, groups=groups)
        above = layers >= counts[-1]
        assert above.any() and (~above).any()
        assert np.all(got[:, :, above] == 0.0), (case, groups)
        assert np.count_nonzero(got[:, :, ~above]) > 0
    if c["n_spec"]:  # a species without lines: its K column all zero
        K = r.cols["K"]
        keep = K[0].clone()
        try:
            K[0].zero_()
            got = r.vjp(r.G)
        finally:
            K[0].copy_(keep)
        slot = [i for i, w in enumerate(c["wrt"]) if w != "T"][0]
        assert np.all(got[:, slot] == 0.0)
        others = [i for i in range(len(c["wrt"])) if i != slot]
        assert np.array_equal(got[:, others], r.grad[:, others])


# ------------------------------------------------------------------------------------------------ e. N_angle = 1
def test_single_angle(run):
    r = run(6)
    nZ = r.nZ
    got = r.vjp(r.G, N_angle=1)
    assert np.isnan(got).all()
    got = r.vjp(r.G, groups=(False, False, True), N_angle=1)
    assert np.isnan(got).all()
    got = r.vjp(r.G, groups=(True, True, False), N_angle=1)
    assert np.isfinite(got).all()
    # tau and L-up rows do not involve the streams: the stored J of the 9-angle run has them
    want, scale = cases.contract(r.G[:, :2 * nZ], r.J[:, :, :2 * nZ])
    _within(got, want, scale, "N_angle = 1, tau + Lu")


# ------------------------------------------------------------------------------------------------ f. bit identity
@pytest.mark.parametrize("case", [2, 5])
def test_bit_identity(eng, run, case, monkeypatch):
    r = run(case)
    c = r.c
    again = r.vjp(r.G)
    assert np.array_equal(again, r.grad)
    # any subset and order of layers: the same bits per layer
    rng = np.random.default_rng(case)
    layers = np.asarray(c["layers"])
    for pick in (rng.permutation(layers.size), rng.permutation(layers.size)[:3], np.array([layers.size - 1])):
        got = r.vjp(r.G, layers=layers[pick])
        assert np.array_equal(got, r.grad[:, :, pick]), pick
    # vectors one at a time, and every blocking of them by the engine
    for v in range(c["n_vec"]):
        assert np.array_equal(r.vjp(r.G[v:v + 1])[0], r.grad[v]), v
    n_max = eng._lib.load().rtx_tud_vjp_max_vectors()
    assert c["n_vec"] == n_max + 1
    for group in (1, 2, 3):
        monkeypatch.setattr(eng, "VJP_VEC_GROUP", group)
        assert np.array_equal(r.vjp(r.G), r.grad), group
    # an unpadded G (another leading dimension) and a cotangent given without the vector axis
    assert np.array_equal(r.vjp(r.G, pad=0), r.vjp(r.G, pad=3))
    nZ = r.nZ
    k = r.cols
    one = eng.tud_vjp_from_od(k["OD"], k["ODp"], k["ODm"], H_T, k["K"], k["tau"], r.grid, c["T"], c["Z"], G_tau=r.G[0, :nZ],
                              G_Lu=r.G[0, nZ:2 * nZ], G_Ld=r.G[0, 2 * nZ], **r.kw())
    assert np.array_equal(one.cpu().numpy()[0], r.grad[0])


# ------------------------------------------------------------------------------------------------ g. end to end
def test_compute_tud_vjp_end_to_end():
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
    rng = np.random.default_rng(3)
    n_vec = 2
    g_La = rng.normal(size=(nX, nZ, n_vec))
    g_La[:, 1, 0] = 0.0
    g_Ld = rng.normal(size=(nX, n_vec))
    g_Ld[nX // 4:nX // 2] = 0.0
    Xv, tau_v, La_v, Ld_v, grad = rt.compute_TUD_vjp(lo, hi, {"La": g_La, "Ld": g_Ld}, wrt=wrt, **kw)
    assert np.array_equal(Xv, X) and np.array_equal(tau_v, tau) and np.array_equal(La_v, La) and np.array_equal(Ld_v, Ld)
    assert set(grad) == set(wrt)
    Xj, _, _, _, J = rt.compute_TUD_jacobian(lo, hi, wrt=wrt, **kw)
    G32 = lambda g: g.astype(np.float32).astype(np.float64)  # the cotangent the device is given
    for w in wrt:
        assert grad[w].shape == (nL, n_vec) and grad[w].dtype == np.float64
        dLa, dLd = J[w][1], J[w][2]  # [nX][nZ][nL], [nX][nL]: float64 copies of the stored float32 J
        want = np.einsum("xav,xal->lv", G32(g_La), dLa) + np.einsum("xv,xl->lv", G32(g_Ld), dLd)
        scale = np.einsum("xav,xal->lv", np.abs(G32(g_La)), np.abs(dLa)) + np.einsum("xv,xl->lv", np.abs(G32(g_Ld)), np.abs(dLd))
        if w == 3:  # the synthetic table holds H2O and CO2 lines only: a species without lines, exact zeros
            assert not want.any() and np.all(grad[w] == 0.0)
        else:
            assert np.count_nonzero(want) > 0.5 * want.size
        g_sum = np.abs(G32(g_La)).sum(axis=(0, 1)) + np.abs(G32(g_Ld)).sum(axis=0)  # [n_vec]
        _within(grad[w], want, scale, "end to end, wrt %r" % (w,), g_sum=g_sum[None, :])
    # a torch cotangent (here already on the device) gives the same bits; a single vector drops the vector axis
    t_grad = rt.compute_TUD_vjp(lo, hi, {"La": torch.as_tensor(g_La, device="cuda"), "Ld": torch.as_tensor(g_Ld)}, wrt=wrt, **kw)[4]
    for w in wrt:
        assert np.array_equal(t_grad[w], grad[w])
    one = rt.compute_TUD_vjp(lo, hi, {"La": g_La[..., 1], "Ld": g_Ld[..., 1]}, wrt=wrt, layers=[65, 3, 8], **kw)[4]
    for w in wrt:
        assert one[w].shape == (3,) and np.array_equal(one[w], grad[w][[65, 3, 8], 1])


# ------------------------------------------------------------------------------- h. the Jacobian kernel is untouched
# SHA-256 of the bytes of J (float32, [n_wrt][n_lay][rows][n]) that engine.tud_jacobian_from_od gives for cases.make(6),
# recorded on an MI355X from a build of the parent commit f85d30f (before rtx_tud_jac.hip's helpers moved to
# rtx_tud_jac_common.h).
PARENT_J_SHA256 = "76a5e87b1f15f776929d27b5d06684bc374be3c6eacfb842d921403e5dcbf203"


def test_jacobian_bits_are_the_parent_commits(run):
    r = run(6)
    J = r.jacobian().contiguous().cpu().numpy()
    assert J.dtype == np.float32
    assert hashlib.sha256(J.tobytes()).hexdigest() == PARENT_J_SHA256


# ------------------------------------------------------------------------------- i. and so is the adjoint kernel
# The seven non-empty selections of the row groups (tau, L-up, Ld): one instantiation of tud_vjp_kernel each.
SELECTIONS = [(t, u, d) for t in (False, True) for u in (False, True) for d in (False, True)][1:]

# SHA-256 over the concatenated bytes of grad (float64, [n_vec][n_wrt][n_lay]) that engine.tud_vjp_from_od gives for the seven
# SELECTIONS in that order, per case of cases.make; "dod": the same through rtx_tud_vjp_dod on case 1, the derivative given
# as (ODp - ODm) / (2 H_T). Recorded on an MI355X from a build of the parent commit 14c6c52 (before the entry glue of the
# three derivative files moved to rtx_tud_jac_common.h and their scratch to StreamScratch; whoever next moves the sweeps or
# the row factors, which this kernel and tud_jac_kernel each carry, is held to these bits).
PARENT_VJP_SHA256 = {
    1: "1dbc5ea54732bfb058af97b5f12f435f8575e8bf24e2f06066cdd2c595094a71",
    4: "5ee2b63bbc16e287dc8467eaa4c903ee16d92219cd8572c94dd5a658570f33d7",
    6: "e82281be5766d87799e4e584a8773ae2c00bdb4544580293ee4dac90f490cddb",
    "dod": "1dbc5ea54732bfb058af97b5f12f435f8575e8bf24e2f06066cdd2c595094a71",
}


def vjp_bits(r, dOD_dT=None):
    """The hash described above for a Run."""
    k = r.cols
    nZ = r.nZ
    pad = r.c["pad"]
    G = np.asarray(r.G, dtype=np.float32)
    fd = (k["ODp"], k["ODm"]) if dOD_dT is None else (None, None)
    h = hashlib.sha256()
    for tau, up, down in SELECTIONS:
        out = r.eng.tud_vjp_from_od(k["OD"], fd[0], fd[1], H_T, k["K"], k["tau"], r.grid, r.c["T"], r.c["Z"],
                                    G_tau=_dev(G[:, :nZ], pad) if tau else None, G_Lu=_dev(G[:, nZ:2 * nZ], pad) if up else None,
                                    G_Ld=_dev(G[:, 2 * nZ], pad) if down else None, dOD_dT=dOD_dT, **r.kw())
        out = out.contiguous().cpu().numpy()
        assert out.dtype == np.float64 and out.shape == (r.c["n_vec"], len(r.c["wrt"]), len(r.c["layers"]))
        h.update(out.tobytes())
    return h.hexdigest()


def dod_of(c):
    """(ODp - ODm) / (2 H_T) in float32: exact for these inputs (tud_vjp_cases.make)."""
    d32 = (c["ODp"] - c["ODm"]) / np.float32(2.0 * H_T)
    assert d32.dtype == np.float32
    return d32


@pytest.mark.parametrize("case", [1, 4, 6])
def test_vjp_bits_are_the_parent_commits(run, case):
    assert vjp_bits(run(case)) == PARENT_VJP_SHA256[case]


def test_vjp_dod_bits_are_the_parent_commits(run):
    r = run(1)
    assert vjp_bits(r, dOD_dT=_dev(dod_of(r.c), r.c["pad"])) == PARENT_VJP_SHA256["dod"]
