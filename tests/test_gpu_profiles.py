"""GPU: hapi's line-profile functions (radtxfr_amd/hapi.py: pcqsdhc, PROFILE_*, hum1_wei, cpf3, profile_lines) against the
reference's own values, point by point (tests/golden/g16_profiles.npz, tests/make_golden_profiles.py).

The bound of a case is 16 * max(e_ref of that case, E_ord): e_ref is the reference's measured distance from an
extended-precision evaluation of its own formulas (near the PART2 / PART4 and PART3 thresholds it loses up to eight
digits to its own cancellation, and a differently rounded reciprocal or square root moves the same differences), E_ord
the largest e_ref among the ordinary-regime cases, and 16 allows for a kernel that rounds a dozen operations differently.
It is measured against the reference and extended precision, never against the kernel.
"""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from make_golden_profiles import effective_params, reference_args

pytestmark = pytest.mark.gpu

HT_1ATM = (1000.0, 0.0012, 0.05, 0.006, -0.002, 0.0005, 0.01, 0.2)


@pytest.fixture(scope="module")
def hapi():
    from radtxfr_amd import hapi as h
    return h


@pytest.fixture(scope="module")
def g16(golden):
    g = golden("g16_profiles.npz")
    cases = json.loads(str(g["cases"]))
    E_ord = max(float(g["eref_" + c["tag"]]) for c in cases if c["ordinary"])
    return g, cases, E_ord


def case_bound(g, c, E_ord):
    """(reference values, relative bound) of a case; p3_far, which the reference cannot run, is held to `truth` under
    p3_near's bound."""
    if c["has_ref"]:
        return g["ref_" + c["tag"]], 16.0 * max(float(g["eref_" + c["tag"]]), E_ord)
    return g["truth_" + c["tag"]], 16.0 * max(float(g["eref_p3_near"]), E_ord)


def gpu_values(hapi, c, sg):
    out = getattr(hapi, c["fn"])(*reference_args(c, sg))
    return out + 0j if isinstance(out, np.ndarray) else out[0] + 1j * out[1]


def trapezoid(y, x):
    return float(np.sum(0.5 * np.diff(x) * (y[1:] + y[:-1])))


def test_every_golden_case_point_by_point(hapi, g16):
    g, cases, E_ord = g16
    print("\nE_ord = %.2e" % E_ord)
    bad = []
    for c in cases:
        ref, bound = case_bound(g, c, E_ord)
        v = gpu_values(hapi, c, g["sg_" + c["tag"]])
        assert v.shape == ref.shape and v.dtype == np.complex128
        err = float(np.max(np.abs(v - ref) / np.abs(ref)))
        err_re = float(np.max(np.abs(v.real - ref.real)) / np.max(np.abs(ref)))
        e_ref = float(g["eref_" + c["tag"]]) if c["has_ref"] else float("nan")
        print("ACC %-16s %-18s e_ref %.2e  gpu %.2e  gpu_re %.2e  bound %.2e" % (c["tag"], c["fn"], e_ref, err, err_re, bound))
        if not (err <= bound and err_re <= bound):
            bad.append((c["tag"], err, err_re, bound))
    assert not bad, bad


def test_cpf_functions_vs_golden(hapi, g16):
    g, _, E_ord = g16
    for name, fn in (("cpf", hapi.hum1_wei), ("cpf3", hapi.cpf3)):
        re, im = fn(g[name + "_x"], g[name + "_y"])
        ref = g[name + "_ref"]
        err = float(np.max(np.abs(re + 1j * im - ref) / np.abs(ref)))
        bound = 16.0 * max(float(g["eref_" + name]), E_ord)
        print("ACC %-16s e_ref %.2e  gpu %.2e  bound %.2e" % (name, float(g["eref_" + name]), err, bound))
        assert re.dtype == np.float64 and re.shape == ref.shape and err <= bound
    re, im = hapi.hum1_wei(0.5, 0.25)  # scalars give one element
    assert re.shape == (1,) and im.shape == (1,)


def test_limits_against_the_existing_oracle(hapi, g16):
    """PROFILE_VOIGT and PROFILE_SDVOIGT (the new common part, which divides by 1 - 0 A) against oracle.cpu_ref, whose
    SDVoigt sets the common part to A / pi: real parts within the case bound of the complex modulus."""
    from oracle import cpu_ref
    g, cases, E_ord = g16
    for tag, ref_fn, args in (("lim_voigt", cpu_ref.PROFILE_VOIGT, HT_1ATM[:3]), ("lim_sdvoigt", cpu_ref.PROFILE_SDVOIGT, HT_1ATM[:6])):
        sg = g["sg_" + tag]
        c = next(c for c in cases if c["tag"] == tag)
        ref, bound = case_bound(g, c, E_ord)
        want = ref_fn(*args, sg)
        want = want[0] if isinstance(want, tuple) else want
        got = getattr(hapi, c["fn"])(*args, sg)[0]
        err = float(np.max(np.abs(got - want) / np.abs(ref)))
        print("ACC %-16s vs oracle.cpu_ref  gpu_re %.2e  bound %.2e" % (tag, err, bound))
        assert err <= bound


def test_shapes_orders_and_types(hapi):
    rng = np.random.default_rng(7)
    sg = np.linspace(999.0, 1001.0, 700)  # two full workgroups of 256 points and a tail of 188
    re, im = hapi.pcqsdhc(*HT_1ATM, sg)
    assert re.shape == im.shape == (700,) and re.dtype == im.dtype == np.float64 and np.all(np.isfinite(re)) and np.all(np.isfinite(im))
    for i in (0, 255, 256, 511, 512, 699):  # n = 1, a Python scalar: shape (1,), the same bits
        r1, i1 = hapi.pcqsdhc(*HT_1ATM, float(sg[i]))
        assert r1.shape == i1.shape == (1,) and r1[0] == re[i] and i1[0] == im[i]
    r1, i1 = hapi.PROFILE_HT(*HT_1ATM, np.float64(sg[3]))
    assert r1.shape == (1,) and r1[0] == re[3] and i1[0] == im[3]
    r1, i1 = hapi.PROFILE_HTP(*HT_1ATM, [sg[5]])
    assert r1.shape == (1,) and r1[0] == re[5] and i1[0] == im[5]
    # descending, and shuffled with repeats: the same values, permuted, bit for bit
    rd, idd = hapi.pcqsdhc(*HT_1ATM, sg[::-1])
    assert np.array_equal(rd, re[::-1]) and np.array_equal(idd, im[::-1])
    perm = rng.integers(0, 700, 900)
    rp, ip = hapi.pcqsdhc(*HT_1ATM, sg[perm])
    assert np.array_equal(rp, re[perm]) and np.array_equal(ip, im[perm])
    rl, il = hapi.pcqsdhc(*HT_1ATM, tuple(sg[:7].tolist()))
    assert np.array_equal(rl, re[:7]) and np.array_equal(il, im[:7])
    # a torch tensor in: tensors out on the same device
    dev = torch.device("cuda", torch.cuda.current_device())
    rt, it = hapi.pcqsdhc(*HT_1ATM, torch.as_tensor(sg, device=dev))
    assert isinstance(rt, torch.Tensor) and rt.device == dev and it.device == dev and rt.dtype == torch.float64
    assert np.array_equal(rt.cpu().numpy(), re) and np.array_equal(it.cpu().numpy(), im)
    rc, _ = hapi.PROFILE_VOIGT(1000.0, 0.0012, 0.05, torch.as_tensor(sg[:9]))
    assert isinstance(rc, torch.Tensor) and rc.device.type == "cpu" and rc.shape == (9,)
    lo = hapi.PROFILE_LORENTZ(1000.0, 0.05, torch.as_tensor(sg, device=dev))
    assert isinstance(lo, torch.Tensor) and lo.device == dev and lo.shape == (700,)
    assert np.array_equal(lo.cpu().numpy(), hapi.PROFILE_LORENTZ(1000.0, 0.05, sg))
    assert hapi.PROFILE_DOPPLER(1000.0, 0.0012, 1000.001).shape == (1,)


def test_leading_dimension_leaves_the_padding_untouched():
    from radtxfr_amd import _lib, engine
    lib = _lib.load()
    dev = engine.device()
    n, ld, nL = 300, 305, 3
    P = torch.zeros((nL, 10), dtype=torch.float64, device=dev)
    P[:, :8] = torch.tensor(HT_1ATM, dtype=torch.float64, device=dev)
    P[:, 0] += torch.arange(nL, device=dev) * 0.25
    sg = torch.linspace(999.0, 1001.0, n, dtype=torch.float64, device=dev)
    for kind in (engine.LS_PCQSDHC, engine.LS_LORENTZ, engine.LS_DOPPLER):
        re = torch.full((nL, ld), -7.0, dtype=torch.float64, device=dev)
        im = torch.full((nL, ld), -9.0, dtype=torch.float64, device=dev)
        _lib.check(lib.rtx_profile_eval(kind, nL, C.c_void_p(P.data_ptr()), C.c_void_p(sg.data_ptr()), n, C.c_void_p(re.data_ptr()),
                                        C.c_void_p(im.data_ptr()), ld, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        want_re, want_im = engine.profile_eval(kind, P, sg)
        assert torch.equal(re[:, :n], want_re) and torch.equal(im[:, :n], want_im)
        assert bool(torch.all(re[:, n:] == -7.0)) and bool(torch.all(im[:, n:] == -9.0))
        re2 = torch.full((nL, ld), -7.0, dtype=torch.float64, device=dev)  # out_im = NULL
        _lib.check(lib.rtx_profile_eval(kind, nL, C.c_void_p(P.data_ptr()), C.c_void_p(sg.data_ptr()), n, C.c_void_p(re2.data_ptr()),
                                        None, ld, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        assert torch.equal(re2, re)


def _lines_from_golden(cases, nL):
    """nL parameter sets drawn from the golden cases in turn, all on ht_1atm's centre, so that neighbouring workgroups (one
    line each) take different PARTs."""
    pool = [effective_params(c) for c in cases if c["fn"] == "pcqsdhc" and c["tag"] != "p3_far"]
    rows = [pool[k % len(pool)] for k in range(nL)]
    cols = [np.array([r[j] for r in rows]) for j in range(8)]
    cols[0] = 1000.0 + 0.01 * np.arange(nL)
    return cols


@pytest.mark.parametrize("nL", [1, 9, 70])
def test_profile_lines_equals_the_one_line_calls(hapi, g16, nL):
    _, cases, _ = g16
    cols = _lines_from_golden(cases, nL)
    sg = np.linspace(999.5, 1001.5, 300)
    re, im = hapi.profile_lines(sg, *cols)
    assert re.shape == im.shape == (nL, 300)
    for l in range(nL):
        r1, i1 = hapi.pcqsdhc(*[complex(c[l]) if j == 7 else float(c[l]) for j, c in enumerate(cols)], sg)
        assert np.array_equal(re[l], r1) and np.array_equal(im[l], i1), l
    if nL == 9:
        lo, lo_im = hapi.profile_lines(sg, cols[0], Gam0=cols[2], profile="LORENTZ")
        do, _ = hapi.profile_lines(sg, cols[0], cols[1], profile="DOPPLER")
        assert not np.any(lo_im)
        for l in range(nL):
            assert np.array_equal(lo[l], hapi.PROFILE_LORENTZ(cols[0][l], cols[2][l], sg))
            assert np.array_equal(do[l], hapi.PROFILE_DOPPLER(cols[0][l], cols[1][l], sg))


@pytest.mark.parametrize("nL", [1, 9, 70, 130])  # 130: more lines than one workgroup stages at a time (128)
def test_profile_lines_weighted_sum(hapi, g16, nL):
    _, cases, _ = g16
    cols = _lines_from_golden(cases, nL)
    rng = np.random.default_rng(nL)
    w = rng.uniform(0.5, 2.0, nL)
    mix = rng.uniform(-0.2, 0.2, nL)
    sg = np.linspace(999.5, 1001.5, 300)
    re, im = hapi.profile_lines(sg, *cols)
    for m in (mix, None):
        got = hapi.profile_lines(sg, *cols, weights=w, mixing=m)
        assert got.shape == (300,) and got.dtype == np.float64
        mm = np.zeros(nL) if m is None else m
        want = np.zeros(300)
        mag = np.zeros(300)
        for l in range(nL):  # the same line order
            want = want + w[l] * (re[l] + mm[l] * im[l])
            mag = mag + abs(w[l]) * (np.abs(re[l]) + abs(mm[l]) * np.abs(im[l]))
        # two orderings / associations of one fp64 sum of nL terms
        assert np.all(np.abs(got - want) <= 4.0 * nL * 2.0 ** -53 * mag), float(np.max(np.abs(got - want) / mag))
        assert np.array_equal(got, hapi.profile_lines(sg, *cols, weights=w, mixing=m))  # bit-identical on a second call
    assert np.array_equal(hapi.profile_lines(sg, *cols, weights=w), hapi.profile_lines(sg, *cols, weights=w, mixing=np.zeros(nL)))
    assert np.array_equal(hapi.profile_lines(sg, *cols, weights=w), hapi.profile_lines(sg, *cols, weights=w, mixing=0.0))
    t = hapi.profile_lines(torch.as_tensor(sg, device="cuda"), *cols, weights=w, mixing=mix)
    assert isinstance(t, torch.Tensor) and t.is_cuda and np.array_equal(t.cpu().numpy(), hapi.profile_lines(sg, *cols, weights=w, mixing=mix))


def test_real_part_integrates_to_one_less_the_tails(hapi, g16):
    """Physics, as a sanity check: the trapezoid integral of Re LS over 900 ... 1100 at ht_1atm is the reference's 0.9997
    (1 less the two Lorentzian tails), and agrees with the same integral of the golden under the case's pointwise bound."""
    g, cases, E_ord = g16
    c = next(c for c in cases if c["tag"] == "ht_1atm_wide")
    ref, bound = case_bound(g, c, E_ord)
    sg = g["sg_ht_1atm_wide"]
    re, _ = hapi.pcqsdhc(*HT_1ATM, sg)
    I, I_ref = trapezoid(re, sg), trapezoid(ref.real, sg)
    print("ACC integral 900-1100: gpu %.15f  reference %.15f" % (I, I_ref))
    assert abs(I_ref - 0.99966) < 5e-5
    assert abs(I - I_ref) <= bound * trapezoid(np.abs(ref), sg)


def test_more_lines_than_one_launch_takes(hapi):
    """rtx_profile_eval puts the line on blockIdx.y, 65 535 per launch, and loops: 65 536 + 3 Lorentz lines at five points
    must land in their own rows on both sides of the cut."""
    nL = 65536 + 3
    sg0 = 1000.0 + 1e-4 * np.arange(nL)
    Gam0 = 0.01 + 1e-7 * np.arange(nL)
    sg = np.array([999.0, 1000.5, 1003.0, 1006.5537, 1010.0])
    re, im = hapi.profile_lines(sg, sg0, Gam0=Gam0, profile="LORENTZ")
    assert re.shape == im.shape == (nL, 5) and not np.any(im)
    want = Gam0[:, None] / (np.pi * (Gam0[:, None] ** 2 + (sg[None, :] - sg0[:, None]) ** 2))
    assert np.all(np.abs(re - want) <= 4 * 2.0 ** -52 * want)  # four roundings apart at the most
    for l in (0, 65534, 65535, 65536, nL - 1):
        assert np.array_equal(re[l], hapi.PROFILE_LORENTZ(sg0[l], Gam0[l], sg)), l
    ht, hi = hapi.profile_lines(sg, sg0[-4:], 0.0012, Gam0[-4:], 0.001, eta=0.1)  # and the same rows through the first launch
    big_re, big_im = hapi.profile_lines(sg, sg0, 0.0012, Gam0, 0.001, eta=0.1)
    assert np.array_equal(big_re[-4:], ht) and np.array_equal(big_im[-4:], hi)
