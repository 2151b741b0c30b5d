"""The case table and the machinery of the stream-contract tests (tests/test_gpu_stream_contract.py on the device,
tests/test_stream_contract_host.py on the CPU); no test in here.

One case per C-ABI function of include/radtxfr_hip.h whose last parameter is `void* stream`: SPECS[name]. A case is
built on the device by SPECS[name].build(v), v = 0, 1, 2 three variants (A, B, C of the tests: other host parameters,
another size). It holds

  inputs    {name: device tensor}   the payload a call reads: spectra, optical depths, tau / La / Ld, emissivities,
                                    cotangents, tangents. The tests hand the call WORKING COPIES of them that hold NaN
                                    until the stream under test has passed its delay, so a kernel that runs early reads NaN;
  outputs   {name: (shape, dtype)}  caller-owned outputs, poisoned the same way before the call;
  host      {name: NumPy array}     the host arrays that cross the ABI (T_h, Ts_h, taps_h, ...). A call gets copies, and
                                    the staging test overwrites those copies as soon as the call has returned;
  call(d, h) -> tensors             d: working inputs and outputs, h: working host arrays. Everything else -- axes, knot
                                    tables, index arrays (kidx, jrange, layer lists, row indices), counts, line records --
                                    is structural: it sits in the closure with its real values from the start, so that a
                                    kernel that runs out of order is never handed an index or a length that could take it
                                    out of bounds (the poison rule);
  scribble  {name: NumPy array}     what a host array is overwritten with where NaN would not be safe if the copy were read
                                    late: arrays that feed window or index arithmetic (layer T and p of a prologue, axes)
                                    get other FINITE values, integer arrays other VALID ones. Default: NaN / zeros.
  check(bits)                       variant 0 only, where the case module the case is built from has an fp64 reference: the
                                    default-stream result against it, at the bound of the GPU test that uses that module
                                    (each figure is printed before it is asserted). A section whose module has none says so.

Functions are reached through their engine / sensor / afit_xs wrapper where one exists and takes device tensors; through
ctypes where there is none, where the wrapper uploads per call (rtx_interp_knots) or runs several entry points that have
cases of their own, and where it makes the whole host array itself (rtx_xs_od's rows and weights, the cube entries' node
tables). Most wrappers hand a contiguous float64 array on as it is (T_h, Ts_h, taps_h, knot_start, layers_h, axes, weights):
the staging test then overwrites the very bytes the library was given. A few rebuild theirs (the dense V of
tud_jvp_from_od, a diluent mix's fraction block, dlnsw of voigt_sum_dT, the dTs groups of band_radiance_srf_jvp): the
library is handed a temporary of the wrapper's that nobody can reach once the wrapper has returned, so the STAGING OF THOSE
FOUR ARRAYS IS NOT TESTED here (whether the allocator hands the freed bytes out again is luck, and the tests do not lean
on it); every other host array of those calls is.
A prologue has no output of its own: its case is prologue + sum on the stream under test; the case of a sum runs its
prologue when it is built, un-delayed, and then only the sum.

may_sync: include/radtxfr_hip.h is the contract. HEADER_SYNC below lists every sentence of it that speaks of
synchronising and whom it binds; may_sync is set exactly for the entries the header says synchronise on EVERY call
("always"). An entry the header lets synchronise only when it allocates or grows ("cold") is warmed by the tests first and
then held to the header's first lines: asynchronous with respect to the host.
"""
import ctypes as C
import os
import re
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "radtxfr_hip.h")
NAN = float("nan")

# ------------------------------------------------------------------------------------------------- the header, parsed
EXCLUDED = {
    "rtx_allgather": "multi-rank: one stream per rank (streams_h); tests/test_gpu_multirank.py",
    "rtx_xs_lut_get_rows": "synchronises `stream` by contract; checked as the read-back of rtx_xs_lut_set_rows' case",
}

# (a phrase of the header that contains "synchronis", kind, the stream entries it binds). kind: "convention" the first
# lines; "setup" creation / free / rtx_lines_set_* calls, which take no stream; "cold" only a call that allocates or grows;
# "always" every call. tests/test_stream_contract_host.py holds this list against the header, occurrence by occurrence.
HEADER_SYNC = [
    ("never allocate, free or synchronise, except", "convention", ()),
    ("others 0; misc/hapi.py:11097-11125). Allocates device memory and synchronises.", "setup", ()),
    ("n_extra = 0 drops it. Allocates device memory and synchronises.", "setup", ()),
    ("to max_points points) and may synchronise; rtx_line_prep only enqueues work.", "setup", ()),
    ("case in which a prologue call allocates and synchronises.", "cold",
     ("rtx_line_prep", "rtx_line_prep_profile", "rtx_line_prep_window", "rtx_line_prep_mix", "rtx_line_prep_dt", "rtx_compute_tud")),
    ("copied into a device buffer owned by the prep object (grow-only: the first call allocates, hence synchronises).\n"
     " * profile RTX_PROFILE_VOIGT / _LORENTZ / _DOPPLER. Follow with rtx_voigt_sum.", "cold", ("rtx_line_prep_window",)),
    ("allocates, hence synchronises), so the caller may free it on return.", "cold", ("rtx_line_prep_axis", "rtx_line_prep_axis_mix")),
    ("the prep object (grow-only: the first call allocates, hence synchronises).\n * rtx_line_prep_mix:", "cold",
     ("rtx_line_prep_mix", "rtx_line_prep_axis_mix")),
    ("in buffers owned by the prep object (grow-only: the first call allocates, hence synchronises), one derivative record", "cold",
     ("rtx_line_prep_dt",)),
    ("allocated and cleared on first use: that call synchronises) as OD_minus", "cold",
     ("rtx_tud_jacobian_dod", "rtx_tud_vjp_dod", "rtx_tud_jvp_dod")),
    ("Calls on one stream share a grow-only workspace; only a call that grows it synchronises. */\n"
     "int rtx_srf_apply(", "cold", ("rtx_srf_apply",)),
    ("Calls on one stream share rtx_srf_apply's grow-only workspace; only a call that grows it synchronises.", "cold", ("rtx_srf_moments",)),
    ("Calls on one stream share a grow-only workspace; only a call that grows it synchronises. */\n"
     "int rtx_srf_radiance_vjp(", "cold", ("rtx_srf_radiance_vjp", "rtx_srf_norms")),
    ("Calls on one stream share a grow-only workspace; only a call that grows it synchronises. */\n"
     "int rtx_srf_radiance_jvp(", "cold", ("rtx_srf_radiance_jvp",)),
    ("n_sets = 0 drops them. Allocates device memory and synchronises.", "setup", ()),
    ("first rtx_ht_prep with work to do (which allocates, hence synchronises, once).", "cold", ("rtx_ht_prep",)),
    ("rtx_cubic_resample without its range check, which reads a flag back from the device and therefore synchronises the\n"
     " * stream", "always", ("rtx_cubic_resample",)),
    ("only the first call with a new slit allocates and synchronises.", "cold", ("rtx_fir_same",)),
    ("zero-filled. Allocates device memory and synchronises.", "setup", ()),
    # (from pageable memory, which is what a caller's NumPy array is and what the case passes; the page-locked form is
    # asynchronous and has a test of its own)
    ("From pageable memory the call synchronises `stream`", "always", ("rtx_xs_lut_set_rows",)),
    ("the inverse, into rows_h; synchronises `stream`.", "always", ("rtx_xs_lut_get_rows",)),
    ("or a larger one, allocates and therefore synchronises; every other call only enqueues.", "cold", ("rtx_xs_od",)),
    ("Environment RADTXFR_COMM=peer|rccl overrides. Allocates and synchronises.", "setup", ()),
]


def header_text():
    with open(HEADER) as f:
        return f.read()


def stream_entries(text=None):
    """Names of the functions include/radtxfr_hip.h declares with a stream as the last parameter (`void* stream`, or
    rtx_allgather's `void* const* streams_h`), in header order."""
    text = header_text() if text is None else text
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = []
    for m in re.finditer(r"\b(rtx_\w+)\s*\(([^;{}()]*)\)\s*;", code):
        last = m.group(2).split(",")[-1].strip()
        if re.fullmatch(r"void\s*\*\s*stream", last) or re.fullmatch(r"void\s*\*\s*const\s*\*\s*streams_h", last):
            out.append(m.group(1))
    return out


def always_sync_entries():
    return {e for _, kind, entries in HEADER_SYNC if kind == "always" for e in entries}


# ------------------------------------------------------------------------------------------------------- case table
class Case:
    def __init__(self, call, inputs=None, outputs=None, host=None, scribble=None, after=None, post=None, check=None, keep=None):
        self.call, self.inputs, self.outputs, self.host = call, dict(inputs or {}), dict(outputs or {}), dict(host or {})
        self.scribble = dict(scribble or {})  # safe replacement values of the staging test, by host-array name
        self.after = after    # called where the staging test overwrites the host arrays: host state the call kept (a runner's block)
        self.post = post      # after the stream has been synchronised: more results (a synchronising read-back)
        self.check = check    # the default-stream result against the reused case module's fp64 reference, at its own bound
        self.keep = keep      # objects the closure needs alive


class Spec:
    def __init__(self, entry, build, workspace, two_streams):
        self.entry, self.build, self.workspace, self.two_streams = entry, build, workspace, two_streams

    @property
    def may_sync(self):
        return self.entry in always_sync_entries()


SPECS = {}
HOST_ARRAY_ENTRIES = set()  # filled by the builders' declarations below: entries whose case has host arrays


def spec(entry, host=False, workspace=False, two_streams=False):
    """Register the builder of `entry`. host: the case has host-array inputs (tests 3 and 4); workspace: a per-stream
    workspace or per-call table the library owns (test 4); two_streams: the header says it is owned per (device, stream)."""
    def reg(fn):
        assert entry not in SPECS, entry
        SPECS[entry] = Spec(entry, fn, workspace or two_streams, two_streams)
        if host:
            HOST_ARRAY_ENTRIES.add(entry)
        return fn
    return reg


# ------------------------------------------------------------------------------------------------------- the delay
class Delay:
    """A bounded spin on the device: torch.cuda._sleep(cycles) where this torch has it, else a chain of large torch.mm.
    Calibrated once with two events on an idle stream. It never waits on the host."""
    FLOOR_MS, CAP_MS, HOST_LIMIT_MS, FACTOR = 60.0, 400.0, 20.0, 20.0

    def __init__(self):
        import torch
        self.torch = torch
        self.sleep = getattr(torch.cuda, "_sleep", None)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            if self.sleep is not None:
                units = 1000000
                self.sleep(1000)
            else:
                self.a = torch.rand((4096, 4096), device="cuda")
                self.b = torch.empty_like(self.a)
                units = 4
                torch.mm(self.a, self.a, out=self.b)
            s.synchronize()
            for _ in range(6):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                self._spin(units)
                e1.record()
                s.synchronize()
                ms = e0.elapsed_time(e1)
                if ms >= 20.0:
                    break
                units = int(units * max(2.0, min(50.0, 30.0 / max(ms, 1e-3))))
        self.units_per_ms = units / ms
        self.calibration = "%s: %d units in %.2f ms" % ("torch.cuda._sleep" if self.sleep is not None else "torch.mm chain", units, ms)

    def _spin(self, units):
        if self.sleep is not None:
            self.sleep(int(units))
        else:
            for _ in range(int(units)):
                self.torch.mm(self.a, self.a, out=self.b)

    def ms_for(self, host_ms, what):
        """D = max(60 ms, 20 x the warmed call's host time), at most 400 ms; a call that needs more than 20 ms fails."""
        assert host_ms <= self.HOST_LIMIT_MS, "%s: the warmed call takes %.2f ms on the host (limit %.0f ms): no delay covers it" \
            % (what, host_ms, self.HOST_LIMIT_MS)
        return min(self.CAP_MS, max(self.FLOOR_MS, self.FACTOR * host_ms))

    def enqueue(self, ms):
        """On the current stream."""
        self._spin(max(1, int(round(ms * self.units_per_ms))))


# ------------------------------------------------------------------------------------------------------- running a case
def flatten(res):
    import torch
    if res is None:
        return []
    if torch.is_tensor(res):
        return [res]
    if isinstance(res, dict):
        res = [res[k] for k in sorted(res)]
    out = []
    for r in res:
        if torch.is_tensor(r) or isinstance(r, (list, tuple, dict)):
            out += flatten(r)
    return out


def bits(t):
    """A host copy of a tensor as integers: NaN compares equal to the same NaN."""
    import torch
    t = t.detach().cpu().contiguous()
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return t.view(view) if t.is_floating_point() else t


def as_float(b):
    """A float tensor that went through bits(), as the NumPy floats it was (the checks against an fp64 reference)."""
    import torch
    return b.view({torch.int16: torch.float16, torch.int32: torch.float32, torch.int64: torch.float64}[b.dtype]).numpy()


def within(got, want, bound, what):
    """|got - want| <= bound element by element (a bound of 0 asks for equality); prints the worst ratio before it asserts."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    print("%s: worst |got - ref| / bound = %.3g" % (what, ratio))
    assert np.isfinite(np.asarray(got, dtype=np.float64)).all() and ratio <= 1.0, (what, ratio)


def same_bits(a, b):
    import torch
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


def describe(a, b):
    """Where two results differ, in a line."""
    import torch
    if len(a) != len(b):
        return "%d tensors against %d" % (len(a), len(b))
    out = []
    for i, (x, y) in enumerate(zip(a, b)):
        if x.shape != y.shape:
            out.append("#%d shape %r / %r" % (i, tuple(x.shape), tuple(y.shape)))
        elif not torch.equal(x, y):
            out.append("#%d: %d of %d elements differ" % (i, int((x != y).sum()), x.numel()))
    return "; ".join(out) or "equal"


def fresh(case):
    """Working copies of a case, poisoned: (device dict, host dict). On the current stream."""
    import torch
    d = {}
    for k, v in case.inputs.items():
        d[k] = torch.full_like(v, NAN)
    for k, (shape, dtype) in case.outputs.items():
        d[k] = torch.full(shape, NAN if dtype.is_floating_point else -77, dtype=dtype, device="cuda")
    return d, {k: np.array(v, copy=True) for k, v in case.host.items()}


def fill(case, d):
    """The real payload into place and the outputs poisoned again, on the current stream."""
    for k, v in case.inputs.items():
        d[k].copy_(v)
    for k, (shape, dtype) in case.outputs.items():
        d[k].fill_(NAN if dtype.is_floating_point else -77)


def overwrite_host(case, h):
    """The staging test's scribble: NaN into every float host array, zeros into every integer one, or the case's own safe
    value. It reaches the arrays the test owns (and, through `after`, a runner's block); a temporary that a wrapper made
    and dropped is out of reach (module docstring)."""
    for k, a in h.items():
        if k in case.scribble:
            a[...] = case.scribble[k]
        elif a.dtype.kind == "f":
            a.fill(np.nan)
        else:
            a.fill(0)
    if case.after is not None:
        case.after()


def issue(case, d, h):
    """One call on the current stream: (results cloned on that stream, host milliseconds of the call alone)."""
    t0 = time.perf_counter()
    res = case.call(d, h)
    ms = (time.perf_counter() - t0) * 1e3
    return res, ms


def finish(case, res):
    """After the stream has been synchronised: the results as bits on the host (with the case's read-back, if it has one)."""
    out = [bits(t) for t in flatten(res)]
    if case.post is not None:
        out += [bits(t) for t in flatten(case.post())]
    return out


def run_plain(case, stream=None):
    """The call on `stream` (default: the default stream) with nothing else going on: (bits, host ms)."""
    import torch
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.default_stream())
    with ctx:
        d, h = fresh(case)
        fill(case, d)
        res, ms = issue(case, d, h)
        torch.cuda.current_stream().synchronize()
        out = finish(case, res)
    torch.cuda.synchronize()
    return out, ms


def run_delayed(cases, stream, delay, ms, scribble=False):
    """The order / asynchrony / staging run: poisoned working copies on the default stream; on `stream` the delay, the
    event `gate`, the real payload, the calls of `cases` back to back. Returns ([bits per case], [gate still pending after
    each call], [host ms of each call])."""
    import torch
    work = []
    with torch.cuda.stream(torch.cuda.default_stream()):
        for c in cases:
            work.append(fresh(c))
    torch.cuda.synchronize()
    gate = torch.cuda.Event()
    res, pending, times = [], [], []
    with torch.cuda.stream(stream):
        delay.enqueue(ms)
        gate.record()
        for c, (d, h) in zip(cases, work):
            fill(c, d)
        for c, (d, h) in zip(cases, work):
            r, t = issue(c, d, h)
            pending.append(not gate.query())
            times.append(t)
            res.append([x.clone() for x in flatten(r)])  # a runner owns its outputs: the next call overwrites them
        if scribble:
            for c, (d, h) in zip(cases, work):
                overwrite_host(c, h)
        stream.synchronize()
        out = [finish(c, r) for c, r in zip(cases, res)]
    torch.cuda.synchronize()
    return out, pending, times


# ------------------------------------------------------------------------------------------------------- fixtures
_FIX = {}


def fixture(name, make):
    if name not in _FIX:
        _FIX[name] = make()
    return _FIX[name]


def release():
    """Close what the builders opened (line tables, cross-section tables)."""
    import torch
    torch.cuda.synchronize()
    for v in _FIX.values():
        for o in (v.values() if isinstance(v, dict) else [v]):
            for m in ("close", "free"):
                if hasattr(o, m) and not isinstance(o, (np.ndarray, dict)):
                    try:
                        getattr(o, m)()
                    except Exception:
                        pass
    _FIX.clear()


def _mods():
    import torch
    from radtxfr_amd import _lib, afit_xs, engine, sensor
    return torch, _lib, _lib.load(), engine, sensor, afit_xs


def dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.array(a, dtype=dtype, copy=True), device="cuda")


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def hp(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- line-sums: dT_cases.kernel_case(1025, 3): one tile + one point, 3 layers, every regime of the kernels --------------
def _ls():
    def make():
        import dT_cases
        _, _, _, engine, _, _ = _mods()
        c = dT_cases.kernel_case(1025, 3)
        tbl = dict(c["tbl"])
        n = np.asarray(tbl["nu"]).size
        tbl["SD_air"] = np.full(n, 0.1)  # read by the speed-dependent prologue alone
        tbl["gamma_self"] = np.full(n, 0.09)
        tbl["n_self"] = np.full(n, 0.6)
        return dict(c=c, tbl=tbl, lines=engine.LineTable(tbl))
    return fixture("ls", make)


# The fp64 references of dT_cases for variant 0, which is kernel_case(1025, 3) as the module makes it (layers, weights and
# shard unchanged). Made once, shared, left unchanged.
#   d sum / dT   dT_cases.linesum_dT, in the metric and at the bound of tests/test_gpu_linesum_dT.py (ratio, TOL 2.85e-5
#                with the floor 1e-3 of the layer's maximum): rtx_line_prep_dt and rtx_voigt_sum_dt.
#   the sum      dT_cases.sum_fixed_window (the oracle's line_params and PROFILE_VOIGT over the device's windows at T_win,
#                with the diluent mix). dT_cases states no device bound for it; the bound here is the one the line-sum path
#                suites hold every Voigt sum to against those same oracle pieces: linesum_metric.pointwise_err <= 1e-5.
#                rtx_line_prep, rtx_voigt_sum, rtx_line_prep_window (T_win = T + 9 K), rtx_line_prep_mix.
# No reference in dT_cases: the Lorentz profile (rtx_line_prep_profile's case), an explicit axis (the rtx_*_axis* entries),
# the speed-dependent sum, and rtx_compute_tud's column (other layers than the module's).
def _ls_want(kind, host):
    def make():
        import dT_cases
        f = _ls()
        c = f["c"]
        rows = []
        for k in range(3):
            T, p = float(c["T"][k]), float(c["p"][k])
            if kind == "dT":
                rows.append(dT_cases.linesum_dT(c["tbl"], c["grid"], T, p, c["weight"], c["dlnw"])[0])
            elif kind == "mix":  # the table of the case, which carries the self-broadening columns
                rows.append(dT_cases.sum_fixed_window(f["tbl"], c["grid"], T, T, p, c["weight"], dil_air=float(host["f_air"][0, k]),
                                                      dil_self=float(host["f_self"][0, k])))
            else:
                rows.append(dT_cases.sum_fixed_window(c["tbl"], c["grid"], T, T + 9.0 if kind == "window" else T, p, c["weight"]))
        want = np.stack(rows)
        want.setflags(write=False)
        return want
    return fixture(("ls_want", kind), make)


def _ls_check(v, kind, what, host=None):
    if v != 0:
        return None

    def check(res):
        import linesum_metric
        want = _ls_want(kind, host)
        got = as_float(res[0]).astype(np.float64)
        assert got.shape == want.shape and np.isfinite(got).all() and np.count_nonzero(want) > 0.5 * want.size
        if kind == "dT":
            zero = want == 0.0
            assert np.all(got[zero] == 0.0), "a structural zero of the definition is not exactly 0"
            den = np.maximum(np.abs(want), 1e-3 * np.max(np.abs(want), axis=1, keepdims=True))
            e, tol = float(np.max(np.where(zero, 0.0, np.abs(got - want) / np.where(den > 0.0, den, 1.0)))), 2.85e-5
        else:
            e, tol = linesum_metric.pointwise_err(got, want), linesum_metric.TOL
        print("%s against dT_cases' fp64 %s: %.3g (bound %.3g)" % (what, "derivative" if kind == "dT" else "sum", e, tol))
        assert e <= tol, (what, e)
    return check


def _ls_variant(v, n_of=(1025, 700, 300)):
    """Layers, weights and the shard of variant v: 3 / 2 / 1 layers, other temperatures and weights, 1025 / 700 / 300 points."""
    _, _, _, engine, _, _ = _mods()
    f = _ls()
    c, lines = f["c"], f["lines"]
    nL = (3, 2, 1)[v]
    T = np.ascontiguousarray(c["T"][:nL] + (0.0, 7.0, -5.0)[v])
    p = np.ascontiguousarray(c["p"][:nL] * (1.0, 0.9, 1.1)[v])
    w = np.ascontiguousarray(np.array([[c["weight"][s]] * nL for s in lines.species], dtype=np.float64) * (1.0, 1.3, 0.7)[v])
    dw = np.ascontiguousarray(np.array([[c["dlnw"][s]] * nL for s in lines.species], dtype=np.float64))
    q, mass = engine.species_factors(lines.species, T, weight=w)
    xmin, xmax, n_total, _, _ = c["grid"]
    grid = engine.Grid(xmin, xmax, n_total, 0, n_of[v])
    host = dict(T=T, p=p, q=np.ascontiguousarray(q), w=w, mass=np.ascontiguousarray(mass))
    # T and p set every line's window: overwritten with other finite values, never NaN (an index must stay in range)
    scribble = dict(T=T * 1.02, p=p * 1.05)
    return lines, grid, nL, host, scribble, dw


def _f32_out(nL, n):
    import torch
    return {"out": ((nL, n), torch.float32)}


def _grid_prologue_case(v, prep, kind="sum"):
    """prologue (a function (lines, grid, nL, h, st) -> None) + the sum `kind` of its records into d["out"]."""
    torch, _lib, lib, engine, _, _ = _mods()
    lines, grid, nL, host, scribble, _ = _ls_variant(v)

    def call(d, h):
        st = engine._stream_ptr()
        prep(lines, grid, nL, h, st)
        plan = lines.plan(nL, grid.n)
        fn = {"sum": lib.rtx_voigt_sum, "sd": lib.rtx_sdvoigt_sum, "dt": lib.rtx_voigt_sum_dt}[kind]
        _lib.check(fn(plan._h, grid.byref(), nL, vp(d["out"]), None, grid.n, st))
        return d["out"]
    return call, lines, grid, nL, host, scribble


def _env(lines, h):
    _, _, _, engine, _, _ = _mods()
    return engine._prologue_inputs(lines, h["T"], h["p"], h["w"], None, h["q"], h["mass"])[1]


@spec("rtx_line_prep", host=True, workspace=True)
def _b_line_prep(v):
    _, _lib, lib, _, _, _ = _mods()

    def prep(lines, grid, nL, h, st):
        env = _env(lines, h)
        _lib.check(lib.rtx_line_prep(lines.plan(nL, grid.n)._h, lines._h, grid.byref(), nL, *(e[1] for e in env), 1.0, 0.0, 0.0, 50.0, 0.0,
                                     1.0, st))
    call, lines, grid, nL, host, scribble = _grid_prologue_case(v, prep)
    return Case(call, outputs=_f32_out(nL, grid.n), host=host, scribble=scribble, check=_ls_check(v, "sum", "rtx_line_prep + rtx_voigt_sum"))


@spec("rtx_line_prep_profile", host=True, workspace=True)
def _b_line_prep_profile(v):
    _, _, _, engine, _, _ = _mods()
    lines, grid, nL, host, scribble, _ = _ls_variant(v)

    def call(d, h):  # Lorentz: another profile than rtx_line_prep's
        engine.voigt_sum(lines, grid, h["T"], h["p"], h["w"], out_f32=d["out"], qratio=h["q"], mass=h["mass"], profile=1)
        return d["out"]
    return Case(call, outputs=_f32_out(nL, grid.n), host=host, scribble=scribble)


@spec("rtx_line_prep_window", host=True, workspace=True)
def _b_line_prep_window(v):
    _, _, _, engine, _, _ = _mods()
    lines, grid, nL, host, scribble, _ = _ls_variant(v)
    host["T_win"] = np.ascontiguousarray(host["T"] + 9.0)
    scribble["T_win"] = host["T_win"] * 0.97

    def call(d, h):
        return engine.voigt_sum_window(lines, grid, h["T"], h["T_win"], h["p"], h["w"], d["out"], qratio=h["q"], mass=h["mass"])
    return Case(call, outputs=_f32_out(nL, grid.n), host=host, scribble=scribble,
                check=_ls_check(v, "window", "rtx_line_prep_window + rtx_voigt_sum"))


def _mix_host(lines, nL, host, v):
    nS = len(lines.species)
    host["f_air"] = np.ascontiguousarray(np.tile(np.linspace(0.8, 0.6, nL) - 0.05 * v, (nS, 1)))
    host["f_self"] = np.ascontiguousarray(1.0 - host["f_air"])


@spec("rtx_line_prep_mix", host=True, workspace=True)
def _b_line_prep_mix(v):
    _, _, _, engine, _, _ = _mods()
    lines, grid, nL, host, scribble, _ = _ls_variant(v)
    _mix_host(lines, nL, host, v)

    def call(d, h):
        engine.voigt_sum(lines, grid, h["T"], h["p"], h["w"], out_f32=d["out"], qratio=h["q"], mass=h["mass"],
                         diluent={"air": h["f_air"], "self": h["f_self"]})
        return d["out"]
    return Case(call, outputs=_f32_out(nL, grid.n), host=host, scribble=scribble,
                check=_ls_check(v, "mix", "rtx_line_prep_mix + rtx_voigt_sum", host))


def _axis_of(grid, v):
    """An explicit non-uniform axis over the grid's span: its points, bent, with a repeat."""
    X = grid.axis()
    X = X + 0.3 * (X[1] - X[0]) * np.sin(np.arange(X.size) * (0.7 + 0.1 * v))
    X = np.sort(X)
    X[5] = X[4]
    return np.ascontiguousarray(X)


def _axis_case(v, mix):
    _, _, _, engine, _, _ = _mods()
    lines, grid, nL, host, scribble, _ = _ls_variant(v)
    host["X"] = _axis_of(grid, v)
    scribble["X"] = np.ascontiguousarray(host["X"][::-1].max() - host["X"][::-1] + host["X"].min())  # ascending, the gaps reversed
    if mix:
        _mix_host(lines, nL, host, v)

    def call(d, h):
        dil = {"air": h["f_air"], "self": h["f_self"]} if mix else None
        engine.voigt_sum_axis(lines, h["X"], h["T"], h["p"], h["w"], out_f32=d["out"], qratio=h["q"], mass=h["mass"], diluent=dil)
        return d["out"]
    return Case(call, outputs=_f32_out(nL, grid.n), host=host, scribble=scribble)


@spec("rtx_line_prep_axis", host=True, workspace=True)
def _b_line_prep_axis(v):
    return _axis_case(v, False)


@spec("rtx_line_prep_axis_mix", host=True, workspace=True)
def _b_line_prep_axis_mix(v):
    return _axis_case(v, True)


@spec("rtx_line_prep_dt", host=True, workspace=True)
def _b_line_prep_dt(v):
    _, _, _, engine, _, _ = _mods()
    lines, grid, nL, host, scribble, dw = _ls_variant(v)
    host["dw"] = dw
    host["dq"] = np.ascontiguousarray(engine.species_dlnq_dT(lines.species, host["T"], weight=host["w"]))

    def call(d, h):
        engine.voigt_sum_dT(lines, grid, h["T"], h["p"], h["w"], d["out"], dlnw_dT=h["dw"], qratio=h["q"], mass=h["mass"], dlnq_dT=h["dq"])
        return d["out"]
    return Case(call, outputs=_f32_out(nL, grid.n), host=host, scribble=scribble, check=_ls_check(v, "dT", "rtx_line_prep_dt + rtx_voigt_sum_dt"))


def _sum_only(v, prologue, sum_call, check=None):
    """The case of a sum: `prologue(lines, grid, nL, host)` runs now, un-delayed; the call is the sum alone."""
    torch, _, _, _, _, _ = _mods()
    lines, grid, nL, host, _, dw = _ls_variant(v)
    host["dw"] = dw
    prologue(lines, grid, nL, host)
    torch.cuda.synchronize()
    plan = lines.plan(nL, grid.n)
    return Case(lambda d, h: sum_call(plan, grid, nL, d["out"]), outputs=_f32_out(nL, grid.n), keep=lines, check=check)


def _scratch(nL, n):
    import torch
    return torch.empty((nL, n), dtype=torch.float32, device="cuda")


@spec("rtx_voigt_sum")
def _b_voigt_sum(v):
    _, _lib, lib, engine, _, _ = _mods()
    return _sum_only(v, lambda lines, grid, nL, h: engine.voigt_sum(lines, grid, h["T"], h["p"], h["w"], out_f32=_scratch(nL, grid.n),
                                                                    qratio=h["q"], mass=h["mass"]),
                     lambda plan, grid, nL, out: (_lib.check(lib.rtx_voigt_sum(plan._h, grid.byref(), nL, vp(out), None, grid.n,
                                                                               engine._stream_ptr())), out)[1],
                     check=_ls_check(v, "sum", "rtx_voigt_sum"))


@spec("rtx_voigt_sum_axis")
def _b_voigt_sum_axis(v):
    _, _lib, lib, engine, _, _ = _mods()
    return _sum_only(v, lambda lines, grid, nL, h: engine.voigt_sum_axis(lines, _axis_of(grid, v), h["T"], h["p"], h["w"],
                                                                         out_f32=_scratch(nL, grid.n), qratio=h["q"], mass=h["mass"]),
                     lambda plan, grid, nL, out: (_lib.check(lib.rtx_voigt_sum_axis(plan._h, nL, vp(out), None, grid.n,
                                                                                    engine._stream_ptr())), out)[1])


@spec("rtx_voigt_sum_dt")
def _b_voigt_sum_dt(v):
    _, _lib, lib, engine, _, _ = _mods()

    def prologue(lines, grid, nL, h):
        engine.voigt_sum_dT(lines, grid, h["T"], h["p"], h["w"], _scratch(nL, grid.n), dlnw_dT=h["dw"], qratio=h["q"], mass=h["mass"],
                            dlnq_dT=engine.species_dlnq_dT(lines.species, h["T"], weight=h["w"]))
    return _sum_only(v, prologue,
                     lambda plan, grid, nL, out: (_lib.check(lib.rtx_voigt_sum_dt(plan._h, grid.byref(), nL, vp(out), None, grid.n,
                                                                                  engine._stream_ptr())), out)[1],
                     check=_ls_check(v, "dT", "rtx_voigt_sum_dt"))


@spec("rtx_sdvoigt_sum")
def _b_sdvoigt_sum(v):
    torch, _lib, lib, engine, _, _ = _mods()
    lines, grid, nL, host, _, _ = _ls_variant(v)
    engine.voigt_sum(lines, grid, host["T"], host["p"], host["w"], out_f64=torch.empty((nL, grid.n), dtype=torch.float64, device="cuda"),
                     qratio=host["q"], mass=host["mass"], profile=3, scale=2.0 ** 70)
    torch.cuda.synchronize()
    plan = lines.plan(nL, grid.n)

    def call(d, h):
        _lib.check(lib.rtx_sdvoigt_sum(plan._h, grid.byref(), nL, None, vp(d["out"]), grid.n, engine._stream_ptr()))
        return d["out"]
    return Case(call, outputs={"out": ((nL, grid.n), torch.float64)}, keep=lines)


@spec("rtx_compute_tud", host=True, workspace=True)
def _b_compute_tud(v):
    """engine.TudRunner.run: prologue + line-sum + TUD in one crossing. The host block the library is given is the runner's
    own (T | p | qratio | weight | mass): the staging test scales it in place after the call (finite: T and p set windows).
    The call has no device payload to withhold, so the order test rests on its outputs: the runner is pointed at the working
    copies of tau, Lu, Ld and OD (TudRunner.set_outputs, its OD attribute), which are poisoned on the stream after the delay
    like any caller-owned output; a kernel of the call that ran early would be overwritten. The records in between belong
    to the prep object, which the variants share: the tests run another variant last before the delayed call, so a sum or
    TUD kernel that ran early would find that variant's records, not its own."""
    torch, _, _, engine, _, _ = _mods()
    lines, grid, nL, _, _, _ = _ls_variant(v)
    run = engine.TudRunner(lines, grid, np.arange(nL) + 0.5, n_layers=nL, Altitudes=(500.0,), theta_r=0.3, N_angle=(9, 30, 2)[v])
    host = dict(T=np.array([296.3, 250.4, 221.7])[:nL] + 3.0 * v, P=np.array([101325.0, 30000.0, 2000.0])[:nL],
                PL=np.array([1.0, 1.0, 2.0])[:nL], MF=np.tile(np.array([[40.0 + 10 * v, 4.0, 1.0]]), (nL, 1)))
    ID = np.array([1, 2, 6])
    nrow = run.shape[0] * run.shape[1]
    outs = {"tau": ((nrow, grid.n), torch.float32), "Lu": ((nrow, grid.n), torch.float32), "Ld": ((grid.n,), torch.float32),
            "OD": ((nL, grid.n), torch.float32)}

    def call(d, h):
        run.set_outputs(d["tau"], d["Lu"], d["Ld"])
        run.OD = d["OD"]
        return run.run(h["T"], h["P"], h["PL"], h["MF"], ID) + (run.OD,)

    def after():
        run._env *= 1.03
    return Case(call, outputs=outs, host=host, scribble={k: a * 1.03 for k, a in host.items()}, after=after, keep=lines)


# ---- TUD and its derivatives: the columns of tests/tud_vjp_cases.py -------------------------------------------------------
def _tud(v):
    """Variant v of the TUD family: configurations 1 (7 layers, 63 points), 6 (9 layers, 1000 points: 4 workgroups) and 3
    (9 layers, 65 points, 16 altitudes) of tud_vjp_cases.CASES; all have T among their wrt entries. Variant 0 is one of the
    configurations the case module flags vs_oracle (6 is not), so its default-stream result is held to the fp64 oracle."""
    import tud_vjp_cases as VC
    _, _, _, engine, _, _ = _mods()
    c = VC.make((1, 6, 3)[v])
    assert v != 0 or c["vs_oracle"]
    n = c["n"]
    grid = engine.Grid(700.0, 701.5, n)
    nZ = c["alts"].size
    inputs = dict(OD=dev(c["OD"]), ODp=dev(c["ODp"]), ODm=dev(c["ODm"]), K=dev(c["K"]),
                  dOD=dev(((c["ODp"].astype(np.float64) - c["ODm"]) / (2 * VC.H_T)).astype(np.float32)))
    if not c["returnOD"]:
        inputs["tau"] = dev(c["tau32"])
    G = c["G"]
    cot = dict(G_tau=dev(G[:, :nZ]), G_Lu=dev(G[:, nZ:2 * nZ]), G_Ld=dev(G[:, 2 * nZ]))
    kw = dict(Altitudes=c["alts"], theta_r=c["theta"], N_angle=c["nA"], returnOD=c["returnOD"], t_pos=c["t_pos"])
    host = dict(T=np.ascontiguousarray(c["T"], dtype=np.float64), layers=np.ascontiguousarray(c["layers"], dtype=np.int32))
    rng = np.random.default_rng(7 + v)
    V = np.ascontiguousarray(rng.normal(size=(min(c["n_vec"], 4), 1 + c["n_spec"], len(c["layers"]))))
    return dict(c=c, grid=grid, inputs=inputs, cot=cot, kw=kw, host=host, V=V, H_T=VC.H_T)


def _pick(d, names):
    return {k: d[k] for k in names if k in d}


# The fp64 oracle of tud_vjp_cases / tud_jvp_cases for variant 0 (oracle_jacobian on the committed oracle.cpu_ref), at the
# bounds of tests/test_gpu_tud_paths.py, test_gpu_tud_vjp.py (b) and test_gpu_tud_jvp.py (a). The _dod forms take
# dOD/dT = (OD+ - OD-) / 2h, which is exact in float32 for these columns, so the same oracle and bounds hold for them.
# The case modules have no reference for the forward rtx_tud (their tau32 is an input).
TOL_L, U32, F32_FLOOR = 1e-5, 2.0 ** -24, 1e-30


def _tud_oracle(f):
    def make():
        import tud_vjp_cases as VC
        from oracle import cpu_ref
        Jo = VC.oracle_jacobian(f["c"], f["grid"].axis(), cpu_ref)
        den = np.maximum(np.maximum(np.abs(Jo), 1e-3 * np.max(np.abs(Jo), axis=-1, keepdims=True)), F32_FLOOR)
        return dict(Jo=Jo, den=den)
    return fixture("tud_oracle", make)


def _stored_jacobian(f):
    """The float32 Jacobian of variant 0 from the device, default stream: bound (b) of the adjoint's test is stated in it."""
    def make():
        torch, _, _, engine, _, _ = _mods()
        i, c = f["inputs"], f["c"]
        J = engine.tud_jacobian_from_od(i["OD"], i["ODp"], i["ODm"], f["H_T"], i["K"], i.get("tau"), f["grid"], f["host"]["T"], c["Z"],
                                        layers=f["host"]["layers"], **f["kw"])
        torch.cuda.synchronize()
        return dict(J=J.double().cpu().numpy())
    return fixture("tud_stored_J", make)["J"]


@spec("rtx_tud", host=True)
def _b_tud(v):
    torch, _, _, engine, _, _ = _mods()
    f = _tud(v)
    c, grid = f["c"], f["grid"]
    nrow, n = c["alts"].size, grid.n
    outs = {"tau": ((nrow, n), torch.float32), "Lu": ((nrow, n), torch.float32), "Ld": ((n,), torch.float32)}

    def call(d, h):
        return engine.tud(d["OD"], grid, h["T"], c["Z"], Altitudes=c["alts"], theta_r=c["theta"], N_angle=c["nA"],
                          returnOD=c["returnOD"], out=(d["tau"], d["Lu"], d["Ld"]))[:3]
    return Case(call, inputs=_pick(f["inputs"], ("OD",)), outputs=outs, host=_pick(f["host"], ("T",)))


def _jac_case(v, dod):
    _, _, _, engine, _, _ = _mods()
    f = _tud(v)
    c, grid, kw = f["c"], f["grid"], f["kw"]

    def call(d, h):
        fd = (None, None, f["H_T"]) if dod else (d["ODp"], d["ODm"], f["H_T"])
        return engine.tud_jacobian_from_od(d["OD"], fd[0], fd[1], fd[2], d["K"], d.get("tau"), grid, h["T"], c["Z"], layers=h["layers"],
                                           dOD_dT=d["dOD"] if dod else None, **kw)
    names = ("OD", "dOD", "K", "tau") if dod else ("OD", "ODp", "ODm", "K", "tau")

    def check(res):
        o = _tud_oracle(f)
        J = as_float(res[0])
        assert J.shape == o["Jo"].shape and np.count_nonzero(o["Jo"]) > 0.3 * o["Jo"].size
        within(J, o["Jo"], TOL_L * o["den"], "rtx_tud_jacobian%s against the fp64 oracle" % ("_dod" if dod else ""))
    return Case(call, inputs=_pick(f["inputs"], names), host=f["host"], check=check if v == 0 else None)


@spec("rtx_tud_jacobian", host=True)
def _b_tud_jacobian(v):
    return _jac_case(v, False)


@spec("rtx_tud_jacobian_dod", host=True)
def _b_tud_jacobian_dod(v):
    return _jac_case(v, True)


def _vjp_case(v, dod):
    _, _, _, engine, _, _ = _mods()
    f = _tud(v)
    c, grid, kw = f["c"], f["grid"], f["kw"]
    cot = {k: t[:4].contiguous() for k, t in f["cot"].items()}  # one launch group of vectors

    def call(d, h):
        fd = (None, None, f["H_T"]) if dod else (d["ODp"], d["ODm"], f["H_T"])
        return engine.tud_vjp_from_od(d["OD"], fd[0], fd[1], fd[2], d["K"], d.get("tau"), grid, h["T"], c["Z"], G_tau=d["G_tau"],
                                      G_Lu=d["G_Lu"], G_Ld=d["G_Ld"], layers=h["layers"], dOD_dT=d["dOD"] if dod else None, **kw)
    names = ("OD", "dOD", "K", "tau") if dod else ("OD", "ODp", "ODm", "K", "tau")
    inputs = _pick(f["inputs"], names)
    inputs.update(cot)

    def check(res):
        import tud_vjp_cases as VC
        o = _tud_oracle(f)
        G = c["G"][:4].astype(np.float64)
        want, _ = VC.contract(G, o["Jo"])
        _, scale_a = VC.contract(G, _stored_jacobian(f))
        bound = TOL_L * np.einsum("vrn,wkrn->vwk", np.abs(G), o["den"]) + 4.0 * U32 * scale_a
        grad = as_float(res[0])
        assert grad.shape == want.shape and grad.dtype == np.float64 and np.count_nonzero(want) > 0.5 * want.size
        within(grad, want, bound, "rtx_tud_vjp%s against the contracted fp64 oracle" % ("_dod" if dod else ""))
    return Case(call, inputs=inputs, host=f["host"], check=check if v == 0 else None)


@spec("rtx_tud_vjp", host=True, two_streams=True)
def _b_tud_vjp(v):
    return _vjp_case(v, False)


@spec("rtx_tud_vjp_dod", host=True, workspace=True)
def _b_tud_vjp_dod(v):
    return _vjp_case(v, True)


def _jvp_case(v, dod):
    _, _, _, engine, _, _ = _mods()
    f = _tud(v)
    c, grid, kw = f["c"], f["grid"], f["kw"]
    host = dict(f["host"], V=f["V"])

    def call(d, h):
        fd = (None, None, f["H_T"]) if dod else (d["ODp"], d["ODm"], f["H_T"])
        o = engine.tud_jvp_from_od(d["OD"], fd[0], fd[1], fd[2], d["K"], d.get("tau"), grid, h["T"], c["Z"], h["V"],
                                   layers=h["layers"], dOD_dT=d["dOD"] if dod else None, **kw)
        return o["tau"], o["La"], o["Ld"]
    names = ("OD", "dOD", "K", "tau") if dod else ("OD", "ODp", "ODm", "K", "tau")

    def check(res):
        import tud_jvp_cases as JC
        from oracle import cpu_ref
        want, S, _ = JC.reference(c, grid.axis(), cpu_ref, f["V"])
        tau, La, Ld = (as_float(t).astype(np.float64) for t in res[:3])
        got = np.concatenate([tau, La, Ld[:, None, :]], axis=1)
        assert got.shape == want.shape and np.count_nonzero(want) > 0.3 * want.size
        within(got, want, TOL_L * S + U32 * np.abs(want), "rtx_tud_jvp%s against the fp64 oracle's J v" % ("_dod" if dod else ""))
    # (V is checked finite on entry, so the scribble is finite)
    return Case(call, inputs=_pick(f["inputs"], names), host=host, scribble={"V": -2.0 * f["V"]}, check=check if v == 0 else None)


@spec("rtx_tud_jvp", host=True, two_streams=True)
def _b_tud_jvp(v):
    return _jvp_case(v, False)


@spec("rtx_tud_jvp_dod", host=True, workspace=True)
def _b_tud_jvp_dod(v):
    return _jvp_case(v, True)


# ---- response-table sensor stage: srf_fused_cases.case(CH, K, "coarse"), nE = 3 ---------------------------------------------
# References: rtx_srf_apply, rtx_srf_moments (+ rtx_band_mix) and rtx_srf_pixel_cube (+ rtx_srf_cube_tables, which makes the
# table that case reads) have an fp64 form in srf_fused_cases / srf_cube_cases, rtx_srf_radiance_vjp and _jvp in
# sensor_vjp_cases / sensor_jvp_cases (the same inputs and bands), and variant 0 of each is held to it below, at the bound of
# the GPU test that uses that module. rtx_srf_norms' N is held to sensor_vjp_cases' fp64 N.
def _srf(v):
    """Variant v: the whole grid of 3 CH + 7 points with all 20 bands and the three temperatures of the case module, nE = 3;
    the grid from its second chunk on with three bands, one temperature, nE = 1; the whole grid with seven bands, two
    temperatures, nE = 2."""
    import srf_fused_cases as FC
    torch, _, lib, engine, sensor, _ = _mods()
    CH, K = lib.rtx_srf_chunk_points(), lib.rtx_srf_max_knots()
    c = FC.case(CH, K, "coarse")
    xmin, xmax, n_total = FC.grid_tuple(CH)
    off, n = [(0, n_total), (CH, n_total - CH), (0, n_total)][v]
    pick = [tuple(range(20)), FC.SUBSET, (0, 1, 2, 3, 7, 8, 10)][v]
    nE = (3, 1, 2)[v]
    key = ("srf_sensor", v)
    s = fixture(key, lambda: sensor.Sensor.from_tables([c["tables"][b] for b in pick]))
    sl = slice(off, off + n)
    inputs = dict(tau=dev(c["tau"][sl]), La=dev(c["La"][sl]), Ld=dev(c["Ld"][sl]), E=dev(np.ascontiguousarray(c["E"][:, :nE])))
    Ts = np.array([FC.TS_LIST, (265.0,), (290.0, 310.0)][v], dtype=np.float64)
    return dict(c=c, FC=FC, grid=engine.Grid(xmin, xmax, n_total, off, n), sensor=s, pick=pick, nE=nE, inputs=inputs, Ts=Ts,
                Xk=np.array(c["Xk"]), Xk_d=dev(c["Xk"]), v=v, n=n)


def _with_knot_start(s, h, fn):
    """fn() with the sensor's host knot_start replaced by the working copy h["knot_start"] for the duration of the call."""
    real = s.knot_start
    s.knot_start = h["knot_start"]
    try:
        return fn()
    finally:
        s.knot_start = real


def _srf_host(f):
    return dict(Ts=f["Ts"].copy(), knot_start=np.array(f["sensor"].knot_start, copy=True))


@spec("rtx_srf_apply", host=True, two_streams=True)
def _b_srf_apply(v):
    _, _, _, _, sensor, _ = _mods()
    f = _srf(v)
    s, grid = f["sensor"], f["grid"]
    import torch
    Y = torch.stack([f["inputs"]["tau"], f["inputs"]["La"], f["inputs"]["Ld"]], dim=1).contiguous()  # [nx][3]

    def call(d, h):
        return _with_knot_start(s, h, lambda: sensor.apply_srf(s, d["Y"], grid=grid, wsum=True)[1:])

    def check(res):
        """Variant 0 against the fp64 band average the response-table suites share (tests/test_gpu_srf.py::reference, which
        srf_cube_cases takes too), at that file's bounds: 1e-5 of max |Y| on the live bands, NaN on the dead ones, the
        denominators to 1e-6 and exactly 0 where dead."""
        from test_gpu_srf import reference
        c = f["c"]
        want, den, _ = reference(np.asarray(c["X"]), c["tables"], Y.cpu().numpy())
        got, d_ = as_float(res[0]).astype(np.float64), as_float(res[1]).astype(np.float64)
        dead = den == 0.0
        assert got.shape == want.shape and np.array_equal(np.isnan(got), np.repeat(dead[:, None], 3, axis=1)) and not dead.all()
        e = float(np.max(np.abs(got[~dead] - want[~dead])) / np.max(np.abs(Y.cpu().numpy())))
        ed = float(np.max(np.abs(d_[~dead] / den[~dead] - 1.0)))
        print("rtx_srf_apply against the fp64 band average: %.3g of max |Y| (bound 1e-5), denominators %.3g (bound 1e-6)" % (e, ed))
        assert e <= 1e-5 and ed <= 1e-6 and np.all(d_[dead] == 0.0)
    return Case(call, inputs={"Y": Y}, host=_pick(_srf_host(f), ("knot_start",)), check=check if v == 0 else None)


@spec("rtx_srf_moments", host=True, two_streams=True)
def _b_srf_moments(v):
    """sensor.band_radiance_srf_fused: rtx_srf_moments and rtx_band_mix per temperature. Variant 0 is the case module's
    own configuration: its fp64 direct form is the reference, at the module's bound (1e-5 of the band's largest |L|)."""
    _, _, _, _, sensor, _ = _mods()
    f = _srf(v)
    s, grid, c, FC = f["sensor"], f["grid"], f["c"], f["FC"]

    def call(d, h):
        return _with_knot_start(s, h, lambda: sensor.band_radiance_srf_fused(grid, d["tau"], d["La"], d["Ld"], f["Xk"], d["E"], h["Ts"], s)[1])

    def check(res):
        import torch
        got = res[0].view(torch.float32).numpy()
        want = c["want"][:, :, :f["nE"]]
        assert np.array_equal(np.isnan(got), np.isnan(want))
        live = ~c["dead"]
        e = float(np.max((np.abs(got - want) / FC.band_max(want))[..., live, :]))
        print("rtx_srf_moments + rtx_band_mix against the fp64 direct form: %.3g of the band maximum (bound 1e-5)" % e)
        assert e <= 1e-5
    return Case(call, inputs=f["inputs"], host=_srf_host(f), check=check if v == 0 else None)


@spec("rtx_srf_norms", host=True, workspace=True)
def _b_srf_norms(v):
    """Through ctypes, not sensor.srf_norms: the wrapper allocates N itself, and every input of the entry is structural (knot
    tables; knot_start is read on the host), so a kernel on the wrong stream that ran early would simply write the right
    values. Here N is a caller-owned output, poisoned on the stream after the delay. Variant 0 (all 20 bands, the whole grid)
    against srf_fused_cases' fp64 N, at the 1e-6 tests/test_gpu_srf_fused.py holds rtx_srf_moments' N to."""
    torch, _lib, lib, engine, _, _ = _mods()
    f = _srf(v)
    s, grid = f["sensor"], f["grid"]
    kx, kr = s.on_device(engine.device())
    torch.cuda.synchronize()

    def call(d, h):
        _lib.check(lib.rtx_srf_norms(grid.byref(), len(s), hp(h["knot_start"]), vp(kx), vp(kr), vp(d["N"]), engine._stream_ptr()))
        return d["N"]

    def check(res):
        N, want, live = as_float(res[0]).astype(np.float64), np.asarray(f["c"]["N"]), ~np.asarray(f["c"]["dead"])
        e = float(np.max(np.abs(N[live] / want[live] - 1.0)))
        print("rtx_srf_norms against the fp64 N: %.3g (bound 1e-6)" % e)
        assert N.shape == want.shape and e <= 1e-6 and np.all(N[~live] == 0.0)
    return Case(call, outputs={"N": ((len(s),), torch.float32)}, host=_pick(_srf_host(f), ("knot_start",)), keep=s,
                check=check if v == 0 else None)


@spec("rtx_srf_radiance_vjp", host=True, two_streams=True)
def _b_srf_radiance_vjp(v):
    _, _, _, _, sensor, _ = _mods()
    f = _srf(v)
    s, grid = f["sensor"], f["grid"]
    rng = np.random.default_rng(11 + v)
    g = rng.normal(size=(f["Ts"].size, len(s), f["nE"])).astype(np.float32)
    if v == 0:  # the case module's own configuration and cotangent (NaN on the dead bands): its fp64 adjoint is the reference
        import sensor_vjp_cases as SV
        _, _, lib, _, _, _ = _mods()
        g, oracle = SV.case_adjoint(lib.rtx_srf_chunk_points(), lib.rtx_srf_max_knots(), "coarse", 3, True)
    inputs = dict(f["inputs"], g=dev(g))

    def call(d, h):
        o = _with_knot_start(s, h, lambda: sensor.band_radiance_srf_vjp(grid, d["tau"], d["La"], d["Ld"], f["Xk"], d["E"], h["Ts"], s, d["g"]))
        return tuple(o[k] for k in ("G_tau", "G_La", "G_Ld", "Ts", "emis"))

    def check(res):
        """|got - want| <= k 2^-24 scale element by element, k the counts of tests/test_gpu_sensor_vjp.py (K_ROW, K_DTS, K_DE)."""
        for t, key, k in zip(res, ("G_tau", "G_La", "G_Ld", "dTs", "dE"), (14, 3, 6, 20, 32)):
            within(as_float(t), oracle[key], k * U32 * oracle["scale"][key], "rtx_srf_radiance_vjp %s against the fp64 adjoint (k = %d)" % (key, k))
    return Case(call, inputs=inputs, host=_srf_host(f), check=check if v == 0 else None)


@spec("rtx_srf_radiance_jvp", host=True, two_streams=True)
def _b_srf_radiance_jvp(v):
    _, _, _, _, sensor, _ = _mods()
    f = _srf(v)
    s, grid, n = f["sensor"], f["grid"], f["n"]
    rng = np.random.default_rng(13 + v)
    t32 = lambda *shape: dev(rng.normal(size=shape).astype(np.float32))
    inputs = dict(f["inputs"], d_tau=t32(n) * 0.01, d_La=t32(n) * 0.1, d_Ld=t32(n) * 0.1, dE=t32(f["Xk"].size, f["nE"]) * 0.01)
    host = dict(_srf_host(f), dTs=np.ascontiguousarray(rng.normal(size=f["Ts"].size)))
    if v == 0:  # the case module's own configuration and tangents (all five groups move): its fp64 tangent is the reference
        import sensor_jvp_cases as SJ
        _, _, lib, _, _, _ = _mods()
        tg, want, scale = SJ.case_tangent(lib.rtx_srf_chunk_points(), lib.rtx_srf_max_knots(), "coarse", 3, True, 51)
        inputs.update(d_tau=dev(tg["d_tau"]), d_La=dev(tg["d_La"]), d_Ld=dev(tg["d_Ld"]), dE=dev(tg["d_E"]))
        host["dTs"] = np.array(tg["d_Ts"], dtype=np.float64)

    def check(res):
        """dL on the live bands: |got - want| <= 32 2^-24 scale, the k of tests/test_gpu_sensor_jvp.py for a vector in which
        all five groups move; the dead bands NaN."""
        dL, dead = as_float(res[1]).astype(np.float64), np.asarray(f["c"]["dead"])
        assert dL.shape == want.shape and np.isnan(dL[:, dead, :]).all()
        within(dL[:, ~dead, :], want[:, ~dead, :], 32 * U32 * scale[:, ~dead, :], "rtx_srf_radiance_jvp dL against the fp64 tangent (k = 32)")

    def call(d, h):
        return _with_knot_start(s, h, lambda: sensor.band_radiance_srf_jvp(grid, d["tau"], d["La"], d["Ld"], f["Xk"], d["E"], h["Ts"], s,
                                                                           d_tau=d["d_tau"], d_La=d["d_La"], d_Ld=d["d_Ld"], d_Ts=h["dTs"],
                                                                           d_emis=d["dE"]))
    # (dTs is checked finite on entry, so the scribble is finite)
    return Case(call, inputs=inputs, host=host, scribble={"dTs": -3.0 * host["dTs"]}, check=check if v == 0 else None)


def _srf_node_moments(f, Q):
    """N, C, M [Q][nB][nk], jrange of the variant at Q node temperatures, made now on the default stream."""
    import srf_cube_cases as CC
    torch, _, _, _, sensor, _ = _mods()
    Tq = CC.nodes((285.0, 315.0), Q)
    i = f["inputs"]
    N, Cb, M, jr = sensor.srf_moments(f["grid"], i["tau"], i["La"], i["Ld"], f["Xk_d"], Tq, f["sensor"])
    torch.cuda.synchronize()
    return Tq, N, Cb, M, jr


@spec("rtx_srf_cube_tables")
def _b_srf_cube_tables(v):
    torch, _lib, lib, engine, _, _ = _mods()
    import srf_cube_cases as CC
    f = _srf(v)
    Q, nEnd = (5, 3, 8)[v], (8, 31, 5)[v]
    _, N, Cb, M, jr = _srf_node_moments(f, Q)
    nB, nk = len(f["sensor"]), f["Xk"].size
    End = dev(CC.endmembers(nk, nEnd))

    def call(d, h):
        _lib.check(lib.rtx_srf_cube_tables(vp(d["M"]), vp(jr), nB, Q, nk, vp(d["End"]), nEnd, vp(d["tab"]), engine._stream_ptr()))
        return d["tab"]
    return Case(call, inputs=dict(M=M, End=End), outputs={"tab": ((nEnd, Q, nB), torch.float32)})


@spec("rtx_srf_pixel_cube", host=True)
def _b_srf_pixel_cube(v):
    torch, _lib, lib, engine, _, _ = _mods()
    import srf_cube_cases as CC
    f = _srf(v)
    Q, nEnd, nMix, nPix = (5, 3, 8)[v], (8, 31, 5)[v], (3, 6, 2)[v], (CC.NPIX, 130, 64)[v]
    T_range = (285.0, 315.0)
    Tq, N, Cb, M, jr = _srf_node_moments(f, Q)
    nB, nk = len(f["sensor"]), f["Xk"].size
    End = dev(CC.endmembers(nk, nEnd))
    tab = torch.empty((nEnd, Q, nB), dtype=torch.float32, device="cuda")
    _lib.check(lib.rtx_srf_cube_tables(vp(M), vp(jr), nB, Q, nk, vp(End), nEnd, vp(tab), engine._stream_ptr()))
    torch.cuda.synchronize()
    sc = CC.scene(nPix, nMix, nEnd, T_range, seed=5 + v)
    kidx = dev(sc["kidx"])
    host = dict(T_node=np.ascontiguousarray(np.concatenate([Tq, T_range])))

    def call(d, h):
        _lib.check(lib.rtx_srf_pixel_cube(nB, Q, hp(h["T_node"]), vp(d["N"]), vp(d["C"]), vp(d["tab"]), nEnd, nPix, nMix, vp(kidx), vp(d["frac"]),
                                          vp(d["Tpix"]), vp(d["cube"]), engine._stream_ptr()))
        return d["cube"]

    def check(res):
        """Variant 0 is srf_cube_cases' accuracy case (coarse knots, 3 of 8 endmembers, 5 nodes over 285-315 K): its fp64
        direct form, at the 1e-5 of the band's largest |L| of tests/test_gpu_srf_cube.py. The inputs of this call were made
        by rtx_srf_moments and rtx_srf_cube_tables on the default stream, so the table kernel is held by this check too
        (srf_cube_cases has no reference for the table alone)."""
        want = CC.case(f["c"], "coarse", "mix3_of_8", "285-315_Q5")["want"]
        e = CC.worst(as_float(res[0]).astype(np.float64), want, f["c"]["dead"])
        print("rtx_srf_cube_tables + rtx_srf_pixel_cube against the fp64 direct form: %.3g of the band maximum (bound 1e-5)" % e)
        assert e <= 1e-5
    return Case(call, inputs=dict(N=N, C=Cb, tab=tab, frac=dev(sc["frac"]), Tpix=dev(sc["T"])), outputs={"cube": ((nB, nPix), torch.float32)},
                host=host, check=check if v == 0 else None)


# ---- MAKO sensor stage: tests/sensor_cases.py ----------------------------------------------------------------------------------
# No reference: sensor_cases holds shapes and inputs only; the fp64 forms these kernels are held to are built inside
# tests/test_gpu_sensor_paths.py, case by case. The same goes for rtx_ils (its case is test_gpu_scratch_reuse.py's shape).
@spec("rtx_apparent_radiance")
def _b_apparent_radiance(v):
    """Both kernels in one call: the row kernel (one atmosphere, nE % 4 == 0) and the general one (atmospheres x dT)."""
    import sensor_cases as SC
    _, _, _, engine, _, _ = _mods()
    row = SC.rad_inputs(SC._rad((5, 3, 9)[v], 4, Ls=True), seed=11 + v)
    gen = SC.rad_inputs(SC._rad((5, 4, 7)[v], 3, nA=3, nT=2, Ls=True), seed=12 + v)
    X = {"r": dev(row["X"]), "g": dev(gen["X"])}
    inputs = {}
    for tag, c in (("r", row), ("g", gen)):
        for k in ("emis", "tau", "La", "Ld", "Ts"):
            inputs[tag + k] = dev(c[k])
    inputs["gdT"] = dev(gen["dT"])

    def call(d, h):
        a = engine.apparent_radiance(X["r"], d["remis"], d["rTs"], d["rtau"], d["rLa"], d["rLd"], return_Ls=True)
        b = engine.apparent_radiance(X["g"], d["gemis"], d["gTs"], d["gtau"], d["gLa"], d["gLd"], dT=d["gdT"], return_Ls=True)
        return a + b
    return Case(call, inputs=inputs)


@spec("rtx_interp_knots")
def _b_interp_knots(v):
    import sensor_cases as SC
    torch, _lib, lib, engine, _, _ = _mods()
    case = SC.INTERP_CASES[("nS4", "nx65", "on_knots")[v]]
    g, X = SC.interp_axis(case)
    grid = engine.Grid(*g)
    Xk = SC.interp_knots_axis(case["knots"])
    Xk_d = dev(Xk)
    nS = case["nS"]
    F = dev(np.random.default_rng(3 + v).uniform(0.5, 1.0, (Xk.size, nS)).astype(np.float32))

    def call(d, h):
        _lib.check(lib.rtx_interp_knots(grid.byref(), None, grid.n, vp(Xk_d), Xk.size, vp(d["F"]), nS, vp(d["out"]), engine._stream_ptr()))
        return d["out"]
    return Case(call, inputs={"F": F}, outputs={"out": ((grid.n, nS), torch.float32)})


def _bbm(v):
    import sensor_cases as SC
    _, _, _, engine, _, _ = _mods()
    knots, kind = SC.BBM_CASES[(0, 3, 1)[v]]
    Xk = SC.bbm_knot_sets()[knots]
    centre, sigma, _ = SC.bbm_bands(knots, kind)
    d = SC.bbm_inputs(seed=21 + v)
    return dict(grid=engine.Grid(*SC.BBM_GRID), kind=kind, Xk=Xk, Xk_d=dev(Xk), c_d=dev(centre), s_d=dev(sigma), nB=centre.size,
                inputs={k: dev(a) for k, a in d.items()}, Ts=SC.BBM_TS + v)


def _moment_outputs(f, rows):
    import torch
    nB, nk = f["nB"], f["Xk"].size
    return {"N": ((nB,), torch.float32), "C": ((nB,), torch.float32), "M": ((rows, nB, nk), torch.float32), "jr": ((nB, 2), torch.int32)}


@spec("rtx_band_moments")
def _b_band_moments(v):
    _, _lib, lib, engine, _, _ = _mods()
    f = _bbm(v)

    def call(d, h):
        _lib.check(lib.rtx_band_moments(f["kind"], f["grid"].byref(), vp(d["tau"]), vp(d["La"]), vp(d["Ld"]), float(f["Ts"]), vp(f["Xk_d"]),
                                        f["Xk"].size, f["nB"], vp(f["c_d"]), vp(f["s_d"]), vp(d["N"]), vp(d["C"]), vp(d["M"]), vp(d["jr"]),
                                        engine._stream_ptr()))
        return d["N"], d["C"], d["M"], d["jr"]
    return Case(call, inputs=f["inputs"], outputs=_moment_outputs(f, 1))


def _basis(f, Q, d, coef, st):
    _, _lib, lib, _, _, _ = _mods()
    _lib.check(lib.rtx_band_basis_moments(f["kind"], f["grid"].byref(), vp(d["tau"]), vp(d["La"]), vp(d["Ld"]), vp(f["Xk_d"]), f["Xk"].size,
                                          f["nB"], vp(f["c_d"]), vp(f["s_d"]), Q, hp(coef), 1.0, vp(d["N"]), vp(d["C"]), vp(d["M"][Q]), vp(d["M"]),
                                          vp(d["jr"]), st))


@spec("rtx_band_basis_moments", host=True)
def _b_band_basis_moments(v):
    _, _, _, engine, sensor, _ = _mods()
    f = _bbm(v)
    Q = (4, 6, 1)[v]
    host = dict(coef=np.ascontiguousarray(sensor.chebyshev_lagrange(Q)[1], dtype=np.float32))

    def call(d, h):
        _basis(f, Q, d, h["coef"], engine._stream_ptr())
        return d["N"], d["C"], d["M"], d["jr"]
    return Case(call, inputs=f["inputs"], outputs=_moment_outputs(f, Q + 1), host=host)


def _basis_now(f, Q):
    """The basis moments of a variant, made now on the default stream: (N, C, M [Q + 1][nB][nk], jrange)."""
    torch, _, _, engine, sensor, _ = _mods()
    d = dict(f["inputs"])
    for k, (shape, dtype) in _moment_outputs(f, Q + 1).items():
        d[k] = torch.zeros(shape, dtype=dtype, device="cuda")
    _basis(f, Q, d, np.ascontiguousarray(sensor.chebyshev_lagrange(Q)[1], dtype=np.float32), engine._stream_ptr())
    torch.cuda.synchronize()
    return d["N"], d["C"], d["M"], d["jr"]


@spec("rtx_band_mix")
def _b_band_mix(v):
    torch, _lib, lib, engine, _, _ = _mods()
    f = _bbm(v)
    N, Cb, M, jr = _basis_now(f, 1)
    nB, nk, nE = f["nB"], f["Xk"].size, (257, 3, 64)[v]
    E = dev(np.random.default_rng(17 + v).uniform(0.55, 1.0, (nk, nE)).astype(np.float32))

    def call(d, h):
        _lib.check(lib.rtx_band_mix(vp(d["N"]), vp(d["C"]), vp(d["M"]), vp(jr), nB, nk, vp(d["E"]), nE, vp(d["out"]), engine._stream_ptr()))
        return d["out"]
    return Case(call, inputs=dict(N=N, C=Cb, M=M[0].contiguous(), E=E), outputs={"out": ((nB, nE), torch.float32)})


@spec("rtx_band_mix_stacked")
def _b_band_mix_stacked(v):
    torch, _lib, lib, engine, _, _ = _mods()
    f = _bbm(v)
    Q = (4, 6, 1)[v]
    _, _, M, jr = _basis_now(f, Q)
    nB, nk, nEnd = f["nB"], f["Xk"].size, (8, 65, 3)[v]
    E = dev(np.random.default_rng(19 + v).uniform(0.55, 1.0, (nk, nEnd)).astype(np.float32))

    def call(d, h):
        _lib.check(lib.rtx_band_mix_stacked(vp(d["M"]), vp(jr), nB, Q + 1, nk, vp(d["E"]), nEnd, vp(d["tab"]), engine._stream_ptr()))
        return d["tab"]
    return Case(call, inputs=dict(M=M, E=E), outputs={"tab": ((nEnd, Q + 1, nB), torch.float32)})


@spec("rtx_pixel_cube", host=True)
def _b_pixel_cube(v):
    import sensor_cases as SC
    torch, _lib, lib, engine, _, _ = _mods()
    case = SC.CUBE_CASES[("nPix257", "global_unstaged", "nPix65")[v]]
    c = SC.cube_inputs(case, seed=31 + v)
    nB, Q, nEnd, nPix, nMix = case["nB"], case["Q"], case["nEnd"], case["nPix"], case["nMix"]
    c_d, s_d, kidx = dev(c["centre"]), dev(c["sigma"]), dev(c["kidx"])
    inputs = dict(N=dev(c["N"]), C=dev(c["C"]), tab=dev(c["tab"]), frac=dev(c["frac"]), Tpix=dev(c["Tpix"]))

    def call(d, h):
        _lib.check(lib.rtx_pixel_cube(nB, Q, vp(c_d), vp(s_d), 1.0, hp(h["s_node"]), vp(d["N"]), vp(d["C"]), vp(d["tab"]), nEnd, nPix, nMix,
                                      vp(kidx), vp(d["frac"]), vp(d["Tpix"]), vp(d["cube"]), engine._stream_ptr()))
        return d["cube"]
    return Case(call, inputs=inputs, outputs={"cube": ((nB, nPix), torch.float32)}, host=dict(s_node=np.ascontiguousarray(c["s_node"])))


@spec("rtx_ils", two_streams=True)
def _b_ils(v):
    """The one-pass rows form of test_gpu_scratch_reuse.py::test_ils_workspace: the smallest that reaches the workspace."""
    torch, _, _, engine, _, _ = _mods()
    nS, nB = 256, 32
    nx = (120000, 150000, 120000)[v]
    gen = torch.Generator(device="cuda").manual_seed(1 + v)
    Y = torch.rand((nx, nS), dtype=torch.float32, device="cuda", generator=gen) + 0.5
    grid = engine.Grid(700.0, 1400.0, nx)
    centre = torch.linspace(720.0, 1380.0, nB, dtype=torch.float64, device="cuda")
    sigma = torch.full((nB,), 1.6 * 660.0 / (nB - 1), dtype=torch.float64, device="cuda")
    return Case(lambda d, h: engine.ils(0, d["Y"], centre, sigma, grid=grid), inputs={"Y": Y})


# ---- post-processing: tests/resample_cases.py ------------------------------------------------------------------------------------
# rtx_fir_reflect, rtx_cubic_resample, its unchecked form and rtx_cubic_end are held to resample_cases' long-double references.
# rtx_fir_same has no case module: its shape is the issue's (a tile + 1 points, a chunk + 1 taps), so no reference either.
@spec("rtx_fir_reflect", host=True)
def _b_fir_reflect(v):
    import resample_cases as RC
    _, _, _, engine, _, _ = _mods()
    name = ("chunk_%d_mid" % (RC.FIR_CHUNK + 1), "tile_n%d_f32" % (RC.FIR_TILE + 1), "tail_taps5")[v]
    c = RC.FIR_CASES[name]
    x, taps = RC.fir_inputs(name)
    Y = dev(x, dtype=np.float32 if c["dtype"] == "f32" else np.float64)

    def check(res):
        import torch
        got = res[0].view(torch.float64).numpy()
        worst = 0.0
        for r in range(c["rows"]):
            want, ab = RC.fir_reference(x[r], taps, c["centre"])
            worst = max(worst, float(np.max(np.abs(got[r].astype(RC.LD) - want) / ((c["n_taps"] + 1) * RC.U * ab))))
        print("rtx_fir_reflect %s against the long-double sum: %.3g of the bound" % (name, worst))
        assert worst <= 1.0
    return Case(lambda d, h: engine.fir_reflect(d["Y"], h["taps"], c["centre"]), inputs={"Y": Y}, host={"taps": np.ascontiguousarray(taps)},
                check=check)


@spec("rtx_fir_same", host=True)
def _b_fir_same(v):
    """One tile + one point, one chunk of taps + one tap (variants: other taps, other sizes)."""
    _, _, lib, engine, _, _ = _mods()
    tile, chunk = lib.rtx_fir_tile_points(), lib.rtx_fir_chunk_taps()
    n, m = (tile + 1, 300, tile)[v], (chunk + 1, 7, 33)[v]
    rng = np.random.default_rng(23 + v)
    Y = dev(rng.uniform(0.5, 2.0, (2, n)))
    taps = np.ascontiguousarray(rng.uniform(0.1, 1.0, m))
    first, n_out = engine.same_window(n, m)
    return Case(lambda d, h: engine.fir_same(d["Y"], h["taps"], 0.5, first, n_out), inputs={"Y": Y}, host={"taps": taps})


def _cubic(v, checked):
    _, _, _, engine, _, _ = _mods()
    n, n_out, rows = (300, 257, 120)[v], (257, 129, 300)[v], (3, 1, 2)[v]
    x0, h_ = 900.0, 2.0 ** -9
    rng = np.random.default_rng(29 + v)
    y = rng.uniform(0.5, 2.0, (rows, n))
    x = x0 + h_ * rng.uniform(26.0, n - 27.0, n_out)
    Y = dev(y)
    x_out = dev(x)  # structural: every abscissa inside the admitted range

    def check(res):
        """resample_cases.cubic_resample_reference (long double) at the bound of tests/test_gpu_resample_paths.py: K u A(q),
        K = resample_cases.CR_K."""
        import resample_cases as RC
        got, worst = as_float(res[0]), 0.0
        for r in range(rows):
            want, A, inside, _ = RC.cubic_resample_reference(y[r], x0, h_, x)
            assert inside.all() and np.isfinite(got[r]).all()
            worst = max(worst, float(np.max(np.abs(got[r].astype(RC.LD) - want) / (RC.CR_K * RC.U * A))))
        print("rtx_cubic_resample%s against the long-double formula: %.3g of the bound" % ("" if checked else "_unchecked", worst))
        assert worst <= 1.0
    return Case(lambda d, h: engine.cubic_resample(d["Y"], x0, h_, x_out, checked=checked), inputs={"Y": Y}, check=check if v == 0 else None)


@spec("rtx_cubic_resample", two_streams=True)
def _b_cubic_resample(v):
    return _cubic(v, True)


@spec("rtx_cubic_resample_unchecked")
def _b_cubic_resample_unchecked(v):
    return _cubic(v, False)


@spec("rtx_cubic_end")
def _b_cubic_end(v):
    import resample_cases as RC
    torch, _lib, lib, engine, _, _ = _mods()
    name = ("ce_m64_rand_lo", "ce_m5_rand_hi", "ce_whole_m48")[v]
    c = RC.CE_CASES[name]
    y, knots, x = RC.ce_inputs(name)
    k_d, x_d = dev(knots), dev(x)
    Y = dev(y)

    def call(d, h):
        _lib.check(lib.rtx_cubic_end(vp(d["Y"]), c["n"], c["rows"], c["i_first"], c["m"], c["high_end"], c["whole_axis"], vp(k_d), vp(x_d),
                                     c["n_out"], vp(d["out"]), c["n_out"], engine._stream_ptr()))
        return d["out"]

    def check(res):
        """resample_cases.ce_reference (long double) at the bound of tests/test_gpu_resample_paths.py: C u max |y| over the
        local window, C = resample_cases.ce_C()."""
        w = slice(c["i_first"], c["i_first"] + c["m"])
        bound = RC.ce_C() * RC.U * np.max(np.abs(y[:, w]), axis=1)[:, None]
        got = as_float(res[0])
        worst = float(np.max(np.abs(got.astype(RC.LD) - RC.ce_reference(name)) / bound))
        print("rtx_cubic_end %s against the long-double spline: %.3g of the bound" % (name, worst))
        assert np.isfinite(got).all() and worst <= 1.0
    return Case(call, inputs={"Y": Y}, outputs={"out": ((c["rows"], c["n_out"]), torch.float64)}, check=check)


# ---- Hartmann-Tran: the 129-candidate block of tests/test_gpu_ht_sum.py -----------------------------------------------------------
# No reference: tests/test_gpu_ht_sum.py compares with recorded sums of the whole table at its own layers
# (tests/golden/g17_ht_sum.npz), which this 129-line block at other temperatures does not reproduce.
def _ht(v):
    def make():
        from make_golden_ht_sum import HEAD, g17_table
        _, _, _, engine, _, _ = _mods()
        G17 = np.load(os.path.join(ROOT, "tests", "golden", "g17_ht_sum.npz"), allow_pickle=False)
        table = g17_table(G17)
        a = HEAD[0]
        return dict(lines=engine.LineTable({k: np.asarray(col)[a:a + 129].copy() for k, col in table.items()}))
    _, _, _, engine, _, _ = _mods()
    lines = fixture("ht", make)["lines"]
    nL = (1, 2, 1)[v]
    T = np.array([296.0, 150.0])[:nL] + 4.0 * v
    p = np.array([1.0, 0.1])[:nL]
    w = np.ones((len(lines.species), nL))
    q, mass = engine.species_factors(lines.species, T, weight=w)
    X = np.ascontiguousarray(np.linspace(903.0, 903.4, (256, 200, 129)[v]))
    host = dict(X=X, T=np.ascontiguousarray(T), p=np.ascontiguousarray(p), w=w, q=np.ascontiguousarray(q), mass=np.ascontiguousarray(mass))
    scribble = dict(X=np.ascontiguousarray(X + 0.05), T=T * 1.02, p=p * 1.05)  # finite: they set every line's window
    DIL = {"air": 0.5, "self": 0.3, "H2": 0.2}
    return lines, nL, host, scribble, DIL


def _ht_sum(lines, h, DIL, out):
    _, _, _, engine, _, _ = _mods()
    return engine.ht_sum(lines, h["X"], h["T"], h["p"], h["w"], DIL, out_f64=out, omega_wing_hw=15.0, qratio=h["q"], mass=h["mass"])[1]


@spec("rtx_ht_prep", host=True, workspace=True)
def _b_ht_prep(v):
    torch, _, _, _, _, _ = _mods()
    lines, nL, host, scribble, DIL = _ht(v)
    return Case(lambda d, h: _ht_sum(lines, h, DIL, d["out"]), outputs={"out": ((nL, host["X"].size), torch.float64)}, host=host,
                scribble=scribble, keep=lines)


def _ht_after_prologue(v):
    torch, _, _, _, _, _ = _mods()
    lines, nL, host, _, DIL = _ht(v)
    _ht_sum(lines, host, DIL, torch.empty((nL, host["X"].size), dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    return lines, nL, host["X"].size, lines.__dict__["_ht_plan"]


@spec("rtx_ht_sum")
def _b_ht_sum(v):
    torch, _lib, lib, engine, _, _ = _mods()
    lines, nL, nx, plan = _ht_after_prologue(v)

    def call(d, h):
        _lib.check(lib.rtx_ht_sum(plan._h, nL, vp(d["o32"]), vp(d["o64"]), nx, engine._stream_ptr()))
        return d["o32"], d["o64"]
    return Case(call, outputs={"o32": ((nL, nx), torch.float32), "o64": ((nL, nx), torch.float64)}, keep=lines)


@spec("rtx_ht_params")
def _b_ht_params(v):
    torch, _lib, lib, engine, _, _ = _mods()
    lines, nL, nx, plan = _ht_after_prologue(v)

    def call(d, h):
        _lib.check(lib.rtx_ht_params(plan._h, nL - 1, vp(d["params"]), vp(d["strength"]), vp(d["window"]), engine._stream_ptr()))
        return d["params"], d["strength"], d["window"]
    return Case(call, outputs={"params": ((lines.n, 10), torch.float64), "strength": ((lines.n,), torch.float64),
                               "window": ((lines.n, 2), torch.int32)}, keep=lines)


# ---- element-wise entries: a few hundred points each ------------------------------------------------------------------------------
# No case module is reused here (the issue asks for a few hundred points each), so there is no reference to hold them to.
def _profile_params(v):
    rng = np.random.default_rng(37 + v)
    nL = (5, 3, 7)[v]
    P = np.zeros((nL, 10))
    P[:, 0] = 1000.0 + rng.uniform(0.0, 1.0, nL)
    P[:, 1] = rng.uniform(1e-3, 3e-3, nL)
    P[:, 2] = rng.uniform(0.01, 0.08, nL)
    P[:, 3] = rng.uniform(0.0, 0.01, nL)
    P[:, 4] = rng.uniform(-0.005, 0.005, nL)
    P[:, 5] = rng.uniform(-0.001, 0.001, nL)
    P[:, 6] = rng.uniform(0.0, 0.02, nL)
    P[:, 7] = rng.uniform(0.0, 0.3, nL)
    P[:, 8] = rng.uniform(-0.1, 0.1, nL)
    n = (300, 257, 64)[v]
    return P, np.sort(rng.uniform(999.5, 1001.5, n)), rng.uniform(0.5, 2.0, nL), rng.uniform(-0.1, 0.1, nL)


@spec("rtx_profile_eval")
def _b_profile_eval(v):
    _, _, _, engine, _, _ = _mods()
    P, sg, _, _ = _profile_params(v)
    return Case(lambda d, h: engine.profile_eval(engine.LS_PCQSDHC, d["P"], d["sg"]), inputs=dict(P=dev(P), sg=dev(sg)))


@spec("rtx_profile_sum")
def _b_profile_sum(v):
    _, _, _, engine, _, _ = _mods()
    P, sg, w_re, w_im = _profile_params(v)
    return Case(lambda d, h: engine.profile_sum(d["P"], d["w_re"], d["w_im"], d["sg"]),
                inputs=dict(P=dev(P), sg=dev(sg), w_re=dev(w_re), w_im=dev(w_im)))


@spec("rtx_cpf_eval")
def _b_cpf_eval(v):
    _, _, _, engine, _, _ = _mods()
    rng = np.random.default_rng(41 + v)
    n = (300, 257, 64)[v]
    x, y = rng.uniform(-20.0, 20.0, n), rng.uniform(0.0, 20.0, n)
    return Case(lambda d, h: engine.cpf_eval(engine.CPF_HUM1_WEI, d["x"], d["y"]) + engine.cpf_eval(engine.CPF_CPF3, d["x"] + 30.0, d["y"]),
                inputs=dict(x=dev(x), y=dev(y)))


@spec("rtx_hapi_spectrum")
def _b_hapi_spectrum(v):
    _, _, _, engine, _, _ = _mods()
    rng = np.random.default_rng(43 + v)
    n = (300, 257, 64)[v]
    K = dev(10.0 ** rng.uniform(-4.0, 0.0, (2, n)), dtype=np.float32 if v == 1 else np.float64)
    X = dev(np.sort(rng.uniform(900.0, 1100.0, n)))
    return Case(lambda d, h: (engine.hapi_spectrum(2, d["K"], 3.0 + v, 296.0, X), engine.hapi_spectrum(0, d["K"], 3.0 + v)), inputs=dict(K=K))


@spec("rtx_planck")
def _b_planck(v):
    _, _, _, engine, _, _ = _mods()
    rng = np.random.default_rng(47 + v)
    n = (300, 257, 64)[v]
    return Case(lambda d, h: engine.planck(d["X"], d["T"]), inputs=dict(X=dev(np.sort(rng.uniform(700.0, 1400.0, n))), T=dev(rng.uniform(200.0, 320.0, 3 + v))))


def _bt_case(v, fn_name):
    torch, _lib, lib, engine, _, _ = _mods()
    rng = np.random.default_rng(53 + v)
    n, m = (300, 257, 64)[v], 3 + v
    X = dev(np.sort(rng.uniform(700.0, 1400.0, n)))
    vals = rng.uniform(1.0, 12.0, (n, m)) if fn_name == "rtx_brightness_temperature" else rng.uniform(200.0, 320.0, (n, m))
    fn = getattr(lib, fn_name)

    def call(d, h):
        _lib.check(fn(vp(X), n, vp(d["V"]), m, 0, NAN, vp(d["out"]), engine._stream_ptr()))
        return d["out"]
    return Case(call, inputs=dict(V=dev(vals)), outputs={"out": ((n, m), torch.float64)})


@spec("rtx_brightness_temperature")
def _b_bt(v):
    return _bt_case(v, "rtx_brightness_temperature")


@spec("rtx_bt2l")
def _b_bt2l(v):
    return _bt_case(v, "rtx_bt2l")


# ---- cross-section tables ----------------------------------------------------------------------------------------------------------
# No case module either: the table is test_gpu_scratch_reuse.py::test_xs_od_terms' shape with random rows.
XS_NX = 1024


def _xs_entries():
    rng = np.random.default_rng(35)
    X = np.linspace(2000.0, 2000.0 + 0.01 * (XS_NX - 1), XS_NX)
    return [dict(ID=ID, T=np.array([250.0, 300.0]), P_atm=np.array([0.5]), X=X, xs=10.0 ** rng.uniform(-24.0, -19.0, (2, 1, XS_NX)))
            for ID in (1, 2)]  # 2 molecules, 4 rows: tests/test_gpu_scratch_reuse.py::test_xs_od_terms


def _xs_lut(name):
    _, _, _, _, _, afit_xs = _mods()
    return fixture(name, lambda: dict(lut=afit_xs.XsLut.from_grids(_xs_entries())))["lut"]


@spec("rtx_xs_od", host=True, two_streams=True)
def _b_xs_od(v):
    torch, _lib, lib, engine, _, _ = _mods()
    lut = _xs_lut("xs")
    nL = (3, 1, 2)[v]
    rng = np.random.default_rng(59 + v)
    T, p, PL = np.array([260.0, 281.3, 299.0])[:nL] + v, np.full(nL, 0.5), np.array([1.0, 0.5, 2.0])[:nL]
    rows, w = lut.layer_terms(T, p, PL, rng.uniform(1.0, 2e4, (nL, 2)), np.array([1, 2]))
    off, n = (0, 4, 1)[v], (XS_NX, 700, 333)[v]

    def call(d, h):
        _lib.check(lib.rtx_xs_od(lut._handle(), off, n, nL, hp(h["rows"]), hp(h["w"]), vp(d["od"]), d["od"].stride(0), engine._stream_ptr()))
        return d["od"]
    # (the other valid value of an index array: every term reads row 0)
    return Case(call, outputs={"od": ((nL, n), torch.float32)}, host=dict(rows=rows, w=w), keep=lut)


@spec("rtx_xs_lut_set_rows", host=True)
def _b_xs_lut_set_rows(v):
    return set_rows_case(v, pinned=False)


def set_rows_case(v, pinned):
    """Two rows from host memory into a table of its own, then rtx_xs_od over exactly those rows on the same stream; after
    the stream has been synchronised the rows are read back with rtx_xs_lut_get_rows. Variants write other rows.
    pinned=False: pageable memory, a host array like any other (the header: such a call synchronises `stream`).
    pinned=True: page-locked memory the case owns and leaves alone, as the header asks: no host array to overwrite."""
    torch, _lib, lib, engine, _, _ = _mods()
    lut = _xs_lut("xs_set")
    row0 = (0, 2, 1)[v]
    rng = np.random.default_rng(61 + v)
    host = dict(rows_h=np.ascontiguousarray(rng.uniform(1.0, 2.0, (2, XS_NX)).astype(np.float32)))
    rows = np.zeros((1, 2, 4), dtype=np.int32)
    rows[0, 0, :] = row0
    rows[0, 1, :] = row0 + 1
    w = np.ascontiguousarray(rng.uniform(0.1, 1.0, (1, 2, 4)).astype(np.float32))

    locked = None
    if pinned:
        locked = torch.empty((2, XS_NX), dtype=torch.float32, pin_memory=True)
        locked.numpy()[...] = host.pop("rows_h")

    def call(d, h):
        st = engine._stream_ptr()
        _lib.check(lib.rtx_xs_lut_set_rows(lut._handle(), row0, 2, C.c_void_p(locked.data_ptr()) if pinned else hp(h["rows_h"]), st))
        _lib.check(lib.rtx_xs_od(lut._handle(), 0, XS_NX, 1, hp(rows), hp(w), vp(d["od"]), XS_NX, st))
        return d["od"]

    def post():
        back = np.empty((2, XS_NX), dtype=np.float32)
        _lib.check(lib.rtx_xs_lut_get_rows(lut._handle(), row0, 2, hp(back), engine._stream_ptr()))
        return torch.from_numpy(back)
    return Case(call, outputs={"od": ((1, XS_NX), torch.float32)}, host=host, post=post, keep=(lut, rows, w, locked))
