"""GPU: the stream contract of include/radtxfr_hip.h -- "calls are asynchronous with respect to the host and never allocate,
free or synchronise" except where an entry says so, host arrays are "staged before returning", workspaces are owned "per
(device, stream)" -- for every entry point that takes a stream (tests/stream_cases.py), on side streams that are BUSY when
the call is made. The value tests pin the default-stream bits of every kernel path to an fp64 oracle; here the yardstick is
bit-equality with the default-stream result, and no tolerance appears anywhere.

On an idle device a wrong stream is invisible. Behind a delay it is deterministic: the payload the call reads is NaN until
the stream under test has passed the delay, and the outputs are poisoned after it, so a kernel, memset or copy enqueued on
any other stream reads NaN or is overwritten; a host array read after the call has returned reads what the test wrote into
it meanwhile.

At most three streams: the default stream, s1 and s2. Every test synchronises the device before it asserts. With
RADTXFR_STREAM_PROFILE=<file> the module writes, per case, whether the call returned before the delay had passed, the warmed
call's host time and the delay D = max(60 ms, 20 x host time) <= 400 ms (profiles/stream_contract.txt is such a file);
only the boolean is asserted."""
import os

import numpy as np
import pytest

import stream_cases as S

pytestmark = pytest.mark.gpu

ENTRIES = sorted(S.SPECS)
HOST = [e for e in ENTRIES if e in S.HOST_ARRAY_ENTRIES]
TWO_CALLS = [e for e in ENTRIES if e in S.HOST_ARRAY_ENTRIES or S.SPECS[e].workspace]
TWO_STREAMS = [e for e in ENTRIES if S.SPECS[e].two_streams]


# the head of the file RADTXFR_STREAM_PROFILE names; everything in that file is written from here
PROFILE_HEAD = """\
# tests/test_gpu_stream_contract.py, written by the module itself with RADTXFR_STREAM_PROFILE=<this file> (torch %s).
# One row per C-ABI entry point that takes a stream (tests/stream_cases.py), variant A:
#   returned before the delay had passed   gate.query() was False right after the warmed call returned, D ms of spinning
#                                          ahead of it on its side stream (the only figure that is asserted: True wherever
#                                          may_sync is False)
#   warmed host ms                         host time of the call through its wrapper, second call on that stream
#   D ms                                   max(60, 20 x host time), at most 400
#   may_sync                               the header says the entry synchronises on every call
#   host arrays                            what the staging test overwrites once the call has returned
# An entry that keeps the host until its stream has caught up leaves the order test blind from that point of the call on:
# what it enqueues afterwards finds the real payload in place whatever stream it is on. rtx_cubic_resample reads its range
# flag back (its kernel is enqueued before that); rtx_xs_lut_set_rows from pageable memory was observed to return only
# once the stream had reached its 2-D copy, while from page-locked memory it returns at once
# (test_set_rows_from_page_locked_memory_is_asynchronous) and the 1-D copies from pageable memory of the other entries do
# not hold the host. The entries that kept the host in this run:
"""


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib
    _lib.load()
    e = dict(torch=torch, s1=torch.cuda.Stream(), s2=torch.cuda.Stream(), delay=S.Delay(), runs={}, rows={})
    yield e
    torch.cuda.synchronize()
    S.release()
    path = os.environ.get("RADTXFR_STREAM_PROFILE")
    if path and e["rows"]:
        with open(path, "w") as f:
            f.write(PROFILE_HEAD % torch.__version__)
            for name in sorted(e["rows"]):
                if "blind" in e["rows"][name]:
                    f.write("#   %s\n" % name)
            f.write("# delay: %s\n# case | returned before the delay had passed | warmed host ms | D ms | may_sync | host arrays\n"
                    % e["delay"].calibration)
            for name in sorted(e["rows"]):
                f.write(e["rows"][name] + "\n")


def _first(env, entry):
    """The runs of tests 1-3 for one entry, made once: reference on the default stream, warm-up and a warmed call on s1,
    the delayed run, and (with host arrays) the delayed run that overwrites them after the call.
    Where the library keeps anything between calls (a workspace, per-call tables, a prep object's records: the entries of
    test 4), the last call on s1 before each delayed run is ANOTHER variant, of another size and with other parameters. A
    kernel of the delayed call that ran early on some other stream and read only library-owned scratch would otherwise
    find there the partials of the identical warm call, which are the right answer; now it finds the other variant's."""
    if entry in env["runs"]:
        return env["runs"][entry]
    torch, s1, delay = env["torch"], env["s1"], env["delay"]
    sp = S.SPECS[entry]
    case = sp.build(0)
    other = sp.build(1) if entry in TWO_CALLS else None
    r = dict(case=case, spec=sp)
    r["ref"], _ = S.run_plain(case)
    r["warm"], _ = S.run_plain(case, s1)          # grows scratch, fills caches
    r["warm2"], r["host_ms"] = S.run_plain(case, s1)  # the warmed call: its host time sets the delay
    r["D"] = delay.ms_for(r["host_ms"], entry)
    if other is not None:
        ref_other, _ = S.run_plain(other)
        assert not S.same_bits(ref_other, r["ref"]), "the two variants give the same bits"
        S.run_plain(other, s1)
    out, pend, _ = S.run_delayed([case], s1, delay, r["D"])
    r["delayed"], r["pending"] = out[0], pend[0]
    if case.host:
        if other is not None:
            S.run_plain(other, s1)
        out, pend, _ = S.run_delayed([case], s1, delay, r["D"], scribble=True)
        r["scribbled"], r["pending_scribbled"] = out[0], pend[0]
    torch.cuda.synchronize()
    env["rows"][entry] = "%-30s | %-5s | %7.3f | %5.0f | %-5s | %s" % (entry, r["pending"], r["host_ms"], r["D"], sp.may_sync,
                                                                       ",".join(sorted(case.host)) or "-")
    if not r["pending"]:  # the call kept the host until the delay had passed: what it enqueued after that point found real inputs
        env["rows"][entry] += " | the order test is blind after the call's blocking point"
    env["runs"][entry] = r
    return r


def _finite_somewhere(env, res):
    """A result that is NaN throughout could not tell a poisoned run from a good one."""
    torch = env["torch"]
    for t in res:
        if t.dtype in (torch.int32, torch.int64) and t.numel():
            f = t.view(torch.float32 if t.dtype == torch.int32 else torch.float64)
            if bool(torch.isfinite(f).any()) and bool((f != 0).any()):
                return True
    return False


@pytest.mark.parametrize("entry", ENTRIES)
def test_order(env, entry):
    """1. Behind a delay on s1, with the payload NaN until s1 has passed the delay and the outputs poisoned after it, the
    call gives the default-stream bits; so does the un-delayed warm-up. Where the reused case module has an fp64 reference
    the default-stream result is held to it at that module's bound."""
    r = _first(env, entry)
    assert r["ref"] and _finite_somewhere(env, r["ref"]), "the reference holds no finite non-zero value"
    if r["case"].check is not None:
        r["case"].check(r["ref"])
    bad = ["%s: %s" % (what, S.describe(r[k], r["ref"])) for k, what in (("warm", "warm-up on s1"), ("warm2", "warmed call on s1"),
                                                                       ("delayed", "behind the delay")) if not S.same_bits(r[k], r["ref"])]
    assert not bad, " | ".join(bad)


@pytest.mark.parametrize("entry", ENTRIES)
def test_asynchrony(env, entry):
    """2. A warmed call returns while the delay ahead of it on its stream is still pending, unless the header says that the
    entry synchronises on every call."""
    r = _first(env, entry)
    print("%s: returned first %s, warmed host time %.3f ms, D %.0f ms" % (entry, r["pending"], r["host_ms"], r["D"]))
    if not r["spec"].may_sync:
        assert r["pending"], "the call returned only after %.0f ms of device work ahead of it on its stream had finished" % r["D"]


def test_set_rows_from_page_locked_memory_is_asynchronous(env):
    """2, for the form of rtx_xs_lut_set_rows the header calls asynchronous: rows in page-locked memory that the caller leaves
    alone. The call returns while the delay is pending, and the rows and the optical depths made from them are the
    default-stream bits (here the order run is not blind: the copy itself waits behind the delay)."""
    torch, s1, delay = env["torch"], env["s1"], env["delay"]
    case = S.set_rows_case(0, pinned=True)
    ref, _ = S.run_plain(case)
    S.run_plain(case, s1)
    warm, ms = S.run_plain(case, s1)
    out, pend, _ = S.run_delayed([case], s1, delay, delay.ms_for(ms, "rtx_xs_lut_set_rows (page-locked)"))
    torch.cuda.synchronize()
    assert S.same_bits(warm, ref) and S.same_bits(out[0], ref), S.describe(out[0], ref)
    assert pend[0], "the call returned only after the delay ahead of it had passed"


@pytest.mark.parametrize("entry", HOST)
def test_host_arrays_are_staged(env, entry):
    """3. Every host array is overwritten as soon as the call has returned, while the delay is pending: the bits do not
    change."""
    r = _first(env, entry)
    assert S.same_bits(r["scribbled"], r["ref"]), "host arrays %s overwritten after the call: %s" \
        % (sorted(r["case"].host), S.describe(r["scribbled"], r["ref"]))


@pytest.mark.parametrize("entry", TWO_CALLS)
def test_two_calls_behind_one_delay(env, entry):
    """4. Delay, call A, call B with other host parameters and another size, all on s1 (both warmed there first, so neither
    grows anything): each equals its own solo reference."""
    torch, s1, delay = env["torch"], env["s1"], env["delay"]
    sp = S.SPECS[entry]
    A, B = sp.build(0), sp.build(1)
    refA, _ = S.run_plain(A)
    refB, _ = S.run_plain(B)
    S.run_plain(A, s1)
    _, tB = S.run_plain(B, s1)
    _, tA = S.run_plain(A, s1)
    out, _, _ = S.run_delayed([A, B], s1, delay, delay.ms_for(tA + tB, entry))
    torch.cuda.synchronize()
    assert not S.same_bits(refA, refB), "the two variants give the same bits"
    assert S.same_bits(out[0], refA), "A: " + S.describe(out[0], refA)
    assert S.same_bits(out[1], refB), "B: " + S.describe(out[1], refB)


@pytest.mark.parametrize("overlap", (False, True), ids=("b_at_once", "b_with_a"))
@pytest.mark.parametrize("entry", TWO_STREAMS)
def test_two_streams(env, entry, overlap):
    """5. The entries that own a workspace, a flag or a per-call table per (device, stream): delay and A on s1, B (other
    inputs, another size) on s2, then C on s1; all three equal their solo references. b_at_once: B is not delayed and runs
    while A waits (a per-call table filled at call time for both streams would hand A the values of B). b_with_a: s2 waits
    for the event recorded after the delay, so B runs alongside A and C (a workspace shared by the two streams)."""
    torch, s1, s2, delay = env["torch"], env["s1"], env["s2"], env["delay"]
    sp = S.SPECS[entry]
    cases = [sp.build(v) for v in range(3)]
    refs = [S.run_plain(c)[0] for c in cases]
    host_ms = 0.0
    for st in (s1, s2):
        for c in cases:
            S.run_plain(c, st)
        host_ms = sum(S.run_plain(c, st)[1] for c in cases)
    work = [S.fresh(c) for c in cases]
    torch.cuda.synchronize()
    gate = torch.cuda.Event()
    res = [None, None, None]
    with torch.cuda.stream(s1):
        delay.enqueue(delay.ms_for(host_ms, entry))
        gate.record()
        for i in (0, 2):
            S.fill(cases[i], work[i][0])
        res[0] = [x.clone() for x in S.flatten(S.issue(cases[0], *work[0])[0])]
    with torch.cuda.stream(s2):
        if overlap:
            s2.wait_event(gate)
        S.fill(cases[1], work[1][0])
        res[1] = [x.clone() for x in S.flatten(S.issue(cases[1], *work[1])[0])]
    with torch.cuda.stream(s1):
        res[2] = [x.clone() for x in S.flatten(S.issue(cases[2], *work[2])[0])]
    torch.cuda.synchronize()
    got = [S.finish(c, r) for c, r in zip(cases, res)]
    torch.cuda.synchronize()
    for name, g, w in zip("ABC", got, refs):
        assert S.same_bits(g, w), "%s: %s" % (name, S.describe(g, w))


# ---------------------------------------------------------------------------------------------- 6. read-only caches
def _cache_cases():
    """{cache: build(tag) -> Case} for the device tables the Python layer caches: the case's call goes through the cache
    under a key no earlier call of the process has used (`tag` makes the key; both uses of a test share it)."""
    import torch
    import sensor_cases as SC
    import srf_fused_cases as FC
    from radtxfr_amd import _lib, engine, sensor
    lib = _lib.load()
    dev = S.dev
    out = {}

    def reduce_cached(tag):
        n, x0, h = 1600, 900.0 + 1e-3 * tag, 0.002
        Y = dev(np.random.default_rng(5).uniform(0.5, 2.0, (3, n)).astype(np.float32))
        return S.Case(lambda d, hh: engine.reduce_resolution_cached(d["Y"], x0, h, n, 9 * h)[1], inputs={"Y": Y})
    out["reduce_resolution_cached"] = reduce_cached

    def bbm(tag, seed=21):
        d = SC.bbm_inputs(seed=seed)
        Xk = SC.bbm_knot_sets()["on_grid"] + 1e-5 * tag  # a knot axis of its own: the key of the three plans
        E = np.random.default_rng(17).uniform(0.55, 1.0, (Xk.size, 3)).astype(np.float32)
        return engine.Grid(*SC.BBM_GRID), {k: dev(a) for k, a in d.items()}, Xk, dev(E)

    def fused_plan(tag):
        grid, i, Xk, E = bbm(tag)
        return S.Case(lambda d, h: sensor.band_radiance_fused(grid, d["tau"], d["La"], d["Ld"], Xk, d["E"], SC.BBM_TS)[1], inputs=dict(i, E=E))
    out["_fused_plan"] = fused_plan

    CH, K = lib.rtx_srf_chunk_points(), lib.rtx_srf_max_knots()
    c = FC.case(CH, K, "coarse")

    def srf_inputs(tag):
        Xk = np.array(c["Xk"]) + 1e-5 * tag
        return (engine.Grid(*FC.grid_tuple(CH)), dict(tau=dev(c["tau"]), La=dev(c["La"]), Ld=dev(c["Ld"]), E=dev(np.ascontiguousarray(c["E"][:, :3]))),
                Xk, sensor.Sensor.from_tables([c["tables"][b] for b in FC.SUBSET]))

    def srf_fused_plan(tag):
        grid, i, Xk, s = srf_inputs(tag)
        s.on_device(engine.device())  # not the cache under test here
        return S.Case(lambda d, h: sensor.band_radiance_srf_fused(grid, d["tau"], d["La"], d["Ld"], Xk, d["E"], list(FC.TS_LIST), s)[1], inputs=i)
    out["_srf_fused_plan"] = srf_fused_plan

    def on_device(tag):
        grid, i, Xk, s = srf_inputs(tag)  # a new Sensor: its knots go to the device on first use
        Y = torch.stack([i["tau"], i["La"], i["Ld"]], dim=1).contiguous()
        return S.Case(lambda d, h: sensor.apply_srf(s, d["Y"], grid=grid)[1], inputs={"Y": Y})
    out["Sensor.on_device"] = on_device

    def cube_plan(tag):
        grid, i, Xk, _ = bbm(tag)
        nEnd, nPix, nMix = 8, 257, 3
        r = np.random.default_rng(31)
        End = dev(r.uniform(0.55, 1.0, (Xk.size, nEnd)).astype(np.float32))
        kidx = dev(r.integers(0, nEnd, (nPix, nMix)).astype(np.int32))
        frac, Tpix = dev(r.uniform(0.1, 1.0, (nPix, nMix)).astype(np.float32)), dev(r.uniform(270.0, 330.0, nPix))
        return S.Case(lambda d, h: sensor.hsi_cube(grid, d["tau"], d["La"], d["Ld"], Xk, d["End"], kidx, d["frac"], d["Tpix"])[1],
                      inputs=dict(tau=i["tau"], La=i["La"], Ld=i["Ld"], End=End, frac=frac, Tpix=Tpix))
    out["_cube_plan"] = cube_plan
    return out


CACHES = ("reduce_resolution_cached", "_fused_plan", "_srf_fused_plan", "_cube_plan", "Sensor.on_device")


@pytest.mark.parametrize("cache", CACHES)
def test_cached_device_tables_across_streams(env, cache):
    """6. A device table the Python layer caches, under a key the process has not seen: first use on s1 behind a delay (it
    builds the table there), second use at once on s2 (it finds the table in the cache), then the default stream once
    everything has finished: the three results are the same bits. The payload of the first use is NaN until s1 has passed
    the delay; the second use has real inputs from the start.
    A regression guard, not a probe that can find a missing event today: every cache under test fills its table with
    torch.as_tensor(<NumPy array>, device=...), a copy from pageable memory that holds the host until s1 has reached it,
    that is until the delay has passed. The second use therefore starts only once the table is complete. The test starts
    to bite the day a table is built by device work (a kernel, a copy from page-locked memory) on the stream of the first
    use."""
    torch, s1, s2, delay = env["torch"], env["s1"], env["s2"], env["delay"]
    build = _cache_cases()[cache]
    tag = 1 + CACHES.index(cache) + 16 * env.setdefault("cache_round", 0)
    first, second = build(tag), build(tag)
    d1, h1 = S.fresh(first)
    d2, h2 = S.fresh(second)
    S.fill(second, d2)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        delay.enqueue(delay.FLOOR_MS)
        S.fill(first, d1)
        r1 = [x.clone() for x in S.flatten(S.issue(first, d1, h1)[0])]
    with torch.cuda.stream(s2):
        r2 = [x.clone() for x in S.flatten(S.issue(second, d2, h2)[0])]
    torch.cuda.synchronize()
    ref, _ = S.run_plain(build(tag))
    got1, got2 = S.finish(first, r1), S.finish(second, r2)
    assert _finite_somewhere(env, ref)
    assert S.same_bits(got1, ref), "first use, on the delayed stream: " + S.describe(got1, ref)
    assert S.same_bits(got2, ref), "second use, at once on another stream: " + S.describe(got2, ref)


def _thin_column(n_layers=32):
    from radtxfr_amd import synthetic
    full = synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
    a = synthetic.c3_atmosphere(n_layers)
    a["MFs_VAL"] = a["MFs_VAL"] * 1e-3
    return full, a


def test_cached_line_tables_and_axis_across_streams(env):
    """6, the two caches behind the drop-ins: hapi's device-table cache (a table name the process has not used) and
    rt._cached_axis (an axis it has not made). First use under a delayed s1, second at once under s2: both return the NumPy
    arrays of the default-stream call."""
    torch, s1, s2, delay = env["torch"], env["s1"], env["s2"], env["delay"]
    from radtxfr_amd import hapi, synthetic
    from radtxfr_amd import radiative_transfer as rt
    full, a = _thin_column(8)
    lo, hi = 1010.0, 1011.0
    sub = synthetic.subset_table(full, lo - 12.0, hi + 12.0)
    hapi.storage2cache_from_columns("stream_contract_cache", sub)
    kw = dict(SourceTables="stream_contract_cache", Environment={"T": 260.0, "p": 0.4}, OmegaRange=[lo, hi], OmegaStep=0.001)
    tud = lambda: rt.compute_TUD(lo, hi, DVOUT=0.00125, line_table=sub, Altitudes=np.asarray([500]), **a)
    got = []
    for st in (s1, s2):
        with torch.cuda.stream(st):
            if st is s1:
                delay.enqueue(delay.FLOOR_MS)
            got.append((hapi.absorptionCoefficient_Voigt(**kw), tud()))
    torch.cuda.synchronize()
    want = (hapi.absorptionCoefficient_Voigt(**kw), tud())
    torch.cuda.synchronize()
    for which, g in zip(("first use, delayed s1", "second use, s2"), got):
        for fn, x, y in zip(("absorptionCoefficient_Voigt", "compute_TUD"), g, want):
            assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(x, y)), (which, fn)
    assert np.isfinite(want[0][1]).all() and want[0][1].max() > 0 and 0.0 <= want[1][1].min() < want[1][1].max() <= 1.0


# ---------------------------------------------------------------------------------------------- 7. the Python drop-ins
def _dropins():
    """{name: function () -> NumPy arrays (or device tensors)} of the drop-ins on small inputs."""
    import torch
    import resample_cases as RC
    import srf_fused_cases as FC
    from radtxfr_amd import _lib, hapi, sensor, synthetic
    from radtxfr_amd import radiative_transfer as rt
    lib = _lib.load()
    full, a = _thin_column(32)
    out = {}
    lo, hi = 1000.0, 1004.0
    sub = synthetic.subset_table(full, lo - 12.0, hi + 12.0)
    kw = dict(DVOUT=0.001, line_table=sub, **a)
    out["compute_TUD"] = lambda: rt.compute_TUD(lo, hi, chunks=1, **kw)
    # the chunked path of test_compute_tud_chunked_equals_unchunked's column, cut to about 3000 points: 3 chunks of a tile
    out["compute_TUD_chunked"] = lambda: rt.compute_TUD(lo, lo + 3.0, chunks=3, Altitudes=np.asarray([2.0, 500.0]), theta_r=np.asarray([0.0, 0.7]), **kw)
    atm = [dict(Ts=a["Ts"] + dT) for dT in (0.0, 2.0, -3.0)]
    flat = lambda res: [x for r in res for x in r]
    out["compute_TUD_batch"] = lambda: flat(rt.compute_TUD_batch(lo, lo + 2.0, atm, **kw))
    out["compute_TUD_batch_reduce"] = lambda: flat(rt.compute_TUD_batch(lo, lo + 2.0, atm, reduce=dict(dX=0.02), **kw))
    hapi.storage2cache_from_columns("stream_contract_dropin", sub)
    out["absorptionCoefficient_Voigt"] = lambda: hapi.absorptionCoefficient_Voigt(
        SourceTables="stream_contract_dropin", Environment={"T": 250.0, "p": 0.3}, OmegaRange=[lo, lo + 1.0], OmegaStep=0.001)
    rng = np.random.default_rng(3)
    Om, cs = np.linspace(1000.0, 1003.0, 3001), rng.uniform(0.0, 1.0, 3001)
    out["convolveSpectrumSame"] = lambda: [np.asarray(v) for v in hapi.convolveSpectrumSame(Om, cs, Resolution=0.05, AF_wing=0.5)[:2]]
    X, Y = RC.axis(1600), RC.spectrum(1600)
    out["reduceResolution"] = lambda: rt.reduceResolution(X, Y, 9 * RC.H)
    CH, K = lib.rtx_srf_chunk_points(), lib.rtx_srf_max_knots()
    c = FC.case(CH, K, "coarse")
    s = sensor.Sensor.from_tables([c["tables"][b] for b in FC.SUBSET])
    Ysp = np.stack([c["tau"], c["La"], c["Ld"]], axis=1)
    out["apply_sensor"] = lambda: rt.apply_sensor(np.array(c["X"]), Ysp, s)
    # hsi_cube_srf takes device tensors: made here, on the default stream, before any delay
    import srf_cube_cases as CC
    from radtxfr_amd import engine
    sc = CC.scene(CC.NPIX, 3, 8, (285.0, 315.0))
    dv = S.dev
    cube_args = (engine.Grid(*FC.grid_tuple(CH)), dv(c["tau"]), dv(c["La"]), dv(c["Ld"]), np.array(c["Xk"]), dv(CC.endmembers(c["Xk"].size, 8)),
                 dv(sc["kidx"]), dv(sc["frac"]), dv(sc["T"]), s)
    torch.cuda.synchronize()
    out["hsi_cube_srf"] = lambda: [sensor.hsi_cube_srf(*cube_args, n_nodes=5, T_range=(285.0, 315.0))[1]]
    # the 1000-point end-to-end case of tests/test_gpu_sensor_vjp.py / test_gpu_sensor_jvp.py, thinned columns
    lo2, hi2 = 1000.0, 1000.5
    sub2 = synthetic.subset_table(full, lo2 - 12.0, hi2 + 12.0)
    sa = rt.StdAtmos
    kw2 = dict(DVOUT=0.0005, line_table=sub2, Altitudes=np.array([8.0]), Zs=sa[:, 1], Ts=sa[:, 5].copy(), Ps=sa[:, 4], PLs=sa[:, 3],
               MFs_VAL=sa[:, 6:9] * 1e6 * 1e-3, MFs_ID=np.array([1, 2, 3]))
    s2 = sensor.Sensor.from_shape([1000.10, 1000.14, 1000.38, 1003.0], 0.06, "triangle")
    Xk = np.array([999.9, 1000.07, 1000.2, 1000.33, 1000.6])
    rng = np.random.default_rng(7)
    E = rng.uniform(0.6, 1.0, (5, 3)).astype(np.float32)
    cot = rng.normal(size=(4, 3)).astype(np.float32)
    tang = {"T": rng.normal(size=66), 1: rng.normal(size=66) * 0.03, "Ts_surface": 0.7, "emis": (rng.normal(size=(5, 3)) * 0.05).astype(np.float32)}

    def vjp():
        X_out, L, grad = rt.compute_band_radiance_vjp(lo2, hi2, s2, Xk, E, 296.0, cot, wrt=("T", 1), **kw2)
        return [X_out, L] + [np.asarray(grad[k]) for k in ("T", 1, "Ts_surface", "emis")]
    out["compute_band_radiance_vjp"] = vjp
    out["compute_band_radiance_jvp"] = lambda: list(rt.compute_band_radiance_jvp(lo2, hi2, s2, Xk, E, 296.0, tang, **kw2))
    return out


DROPINS = ("compute_TUD", "compute_TUD_chunked", "compute_TUD_batch", "compute_TUD_batch_reduce", "absorptionCoefficient_Voigt",
           "convolveSpectrumSame", "reduceResolution", "apply_sensor", "hsi_cube_srf", "compute_band_radiance_vjp", "compute_band_radiance_jvp")


@pytest.fixture(scope="module")
def dropins(env):
    return _dropins()


@pytest.mark.parametrize("name", DROPINS)
def test_dropins_under_a_busy_current_stream(env, dropins, name):
    """7. Each drop-in once on the default stream and once under `with torch.cuda.stream(s1)` behind a delay: the NumPy
    arrays (device tensors: after a synchronise) are the same bits."""
    torch, s1, delay = env["torch"], env["s1"], env["delay"]
    fn = dropins[name]
    host = lambda res: [(v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for v in res]
    want = host(fn())
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        delay.enqueue(delay.FLOOR_MS)
        res = fn()
        s1.synchronize()
        got = host(res)
    torch.cuda.synchronize()
    assert len(got) == len(want) >= 2 or name == "hsi_cube_srf"
    assert any(np.isfinite(w).any() and np.any(w != 0) for w in want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w, equal_nan=True), (name, i)
