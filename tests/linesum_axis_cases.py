"""Line tables, explicit axes and layers that put rtx_line_prep_axis + rtx_voigt_sum_axis on one path at a time. Imported by
the GPU test (tests/test_gpu_linesum_axis_paths.py: every case against the fp64 oracle, point by point) and by the host
test (tests/test_linesum_axis_host.py: each case reaches the labels it names in `expect`, by cpu_ref.axis_census), so the
two cannot drift apart.

A case is a dict: tbl (linesum_cases.table: H2O main isotopologue, chosen centres, widths, strengths), X (the explicit
axis), T, p (per layer), ow / hw (OmegaWing / OmegaWingHW), profile (0 Voigt, 1 Lorentz, 2 Doppler), lineshift (Doppler),
diluent (None or {name: per-layer fractions}), uniform (Grid.from_axis accepts X: the e-cases only) and expect (census
labels that must be non-zero; "!label": must be zero). Every case expects "!outside_bracket".

Windows that must land on an index are set where the prologue's W is the oracle's bit for bit: by OmegaWing (hw = 0), or
by OmegaWingHW * Gamma0 at T = Tref, p = 1 (Gamma0 = gamma_air exactly)."""
import numpy as np

from oracle import cpu_ref

import linesum_cases as LC

table = LC.table


def axis(lo, hi, coarse, fine=()):
    """Coarse steps from lo to hi plus, around each (centre, half, step) of `fine`, steps of `step` within +-half (0.37 of
    a step off the centre: no point on a centre); sorted, no repeats."""
    parts = [np.arange(lo, hi, coarse)]
    for c, half, step in fine:
        parts.append(c + np.arange(-half, half + step / 2, step) + 0.37 * step)
    return np.unique(np.concatenate(parts))


def wavy(x0, step, n, amp=0.5, w=0.7):
    """n strictly increasing points from x0 with steps step * (1 + amp sin(w i)): non-uniform everywhere."""
    i = np.arange(n - 1)
    return np.concatenate([[x0], x0 + np.cumsum(step * (1.0 + amp * np.sin(w * i)))])


def grid_axis(g):
    """The shard axis of a linesum_cases grid tuple (engine.Grid.axis: np.linspace's bits)."""
    xmin, xmax, n_total, offset, n = g
    step = (xmax - xmin) / (n_total - 1)
    X = np.arange(offset, offset + n, dtype=np.float64) * step + xmin
    if n and offset + n == n_total:
        X[-1] = xmax
    return X


def _case(tbl, X, T, p, ow=0.0, hw=50.0, profile=0, lineshift=True, diluent=None, uniform=False, expect=()):
    T, p = np.broadcast_arrays(np.atleast_1d(np.asarray(T, dtype=np.float64)), np.atleast_1d(np.asarray(p, dtype=np.float64)))
    X = np.ascontiguousarray(X, dtype=np.float64)
    assert np.all(X[1:] >= X[:-1])
    return dict(tbl=tbl, X=X, T=T.copy(), p=p.copy(), ow=float(ow), hw=float(hw), profile=int(profile), lineshift=bool(lineshift),
                diluent=diluent, uniform=bool(uniform), expect=tuple(expect) + ("!outside_bracket",))


def _cte_y(nu, gamma, T, p):
    P = cpu_ref.line_params(table([nu], gamma), T, p)
    cte = np.sqrt(np.log(2.0)) / P["GammaD"][0]
    return cte, P["Gamma0"][0] * cte


def _cases():
    C = {}
    # a. profile paths ------------------------------------------------------------------------------------------------
    # Weideman band rows: the widths and pressures of linesum_cases.a_band_*: y = {0.115 ... 9.2} and {1.15 ... 92} at
    # 1000 cm^-1, the same at 6000. Fine steps (a sixth of a Doppler width) +-0.03 / +-0.18 cm^-1 around the centres --
    # the band is +-0.026 / +-0.157 -- and 0.01 cm^-1 steps elsewhere: the row that holds the switch |x| + y = 15 of a
    # 1 <= y < 6 line has every Weideman lane at |z| >= 8 (63 fine points are 3.6 in x), the rows nearer the centre do not
    gam = [0.02, 0.1, 0.15, 0.3, 0.52, 0.61, 1.6]
    for nu0, fstep, half, ps in ((1000.0, 1e-4, 0.03, (0.01, 0.1)), (6000.0, 6e-4, 0.18, (0.06, 0.6))):
        nus = nu0 + 1.0 + 2.0 * np.arange(len(gam)) + 0.123
        X = axis(nu0, nu0 + 14.0, 0.01, [(v, half, fstep) for v in nus])
        C["a_band_%d" % int(nu0)] = _case(table(nus, gam), X, 296.0, ps,
                                          expect=("band_w64", "band_wei32", "band_series_y6", "band_series_ballot",
                                                  "ballot_and_wei32_same_line", "far_rational"))
    # |x| + y = 15 exactly on axis points, left and right of the centre, with their nextafter neighbours and points
    # -+1e-3 (inside the collar: fp64 decides) and -+3e-3 (outside it, inside the band's 0.01 margin: fp32 decides) in x
    # around them; three lines at y ~ 10 (series rows) and three at y ~ 3 (Weideman rows)
    gams = [0.0174, 0.0165, 0.0183, 0.0052, 0.0047, 0.0058]
    nus = 1000.05 + 0.1 * np.arange(len(gams)) + 0.0123
    pts = []
    for v, g in zip(nus, gams):
        cte, y = _cte_y(v, g, 296.0, 1.0)
        for sgn in (-1.0, 1.0):
            e = v + sgn * (15.0 - y) / cte
            pts += [e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf)]
            pts += [v + sgn * (15.0 - y + d) / cte for d in (-3e-3, -1e-3, 1e-3, 3e-3)]
    X = np.unique(np.concatenate([axis(999.9, 1000.8, 0.005, [(v, 0.03, 5e-4) for v in nus]), pts]))
    C["a_switch"] = _case(table(nus, gams), X, 296.0, 1.0,
                          expect=("recheck_in", "recheck_out", "switch_fp32", "band_series_y6", "band_wei32"))
    # the upper standard atmosphere (linesum_cases.a_upper_atmosphere's layers): Doppler-dominated down to y ~ 1e-6
    up = LC.CASES["a_upper_atmosphere"]
    nus = np.array([1000.18, 1000.41, 1000.63]) + 1.23e-4
    X = axis(1000.0, 1000.82, 2e-3, [(v, 0.012, 2e-5) for v in nus])
    C["a_upper_atmosphere"] = _case(table(nus), X, up["T"], up["p"], expect=("band_w64", "far_rational"))
    # Lorentz and Doppler records; lines with delta_air != 0: the window is centred on nu, the profile on nu + shift
    nus = np.array([1000.2, 1000.5, 1000.9]) + 1.23e-4
    tbl = table(nus, [0.07, 0.03, 0.11])
    tbl["delta_air"] = np.array([-0.02, 0.0, 0.015])
    X = axis(999.0, 1002.0, 0.004, [(v, 0.05, 2e-4) for v in nus])
    C["a_lorentz"] = _case(tbl, X, (296.0, 250.0), (1.0, 0.1), profile=1, expect=("lorentz_rows",))
    C["a_doppler"] = _case(tbl, X, (296.0, 250.0), (1.0, 0.1), profile=2, expect=("doppler_w64", "doppler_dropped"))
    C["a_doppler_noshift"] = _case(tbl, X, (296.0, 250.0), (1.0, 0.1), profile=2, lineshift=False,
                                   expect=("doppler_w64", "doppler_dropped"))
    # a Voigt mix of air and self broadening with per-layer fractions (rtx_line_prep_axis_mix)
    tbl = table(nus, [0.07, 0.03, 0.11])
    tbl["gamma_self"] = np.array([0.35, 0.2, 0.45])
    tbl["delta_air"] = np.array([-0.01, 0.0, 0.008])
    C["a_mix"] = _case(tbl, X, (296.0, 260.0, 230.0), (1.0, 0.3, 0.02),
                       diluent={"air": np.array([0.8, 0.5, 0.1]), "self": np.array([0.2, 0.5, 0.9])},
                       expect=("far_rational", "band_wei32", "band_series_y6"))

    # b. abscissa -----------------------------------------------------------------------------------------------------
    # Five tiles of exactly 1024 points whose span X[ib - 1] - X[ia] is 0 (1024 equal points), 0.5, 20, 2000 and 2000
    # cm^-1 (2 cm^-1 steps), each wide one with a line near its END, far from the origin X[ia], sampled by 33 points a
    # quarter of 1/cte apart. 200 K and 0.03 / 0.005 atm: 1 <= y < 6 and y < 1 (widths chosen per line). cte >= 1000
    # needs a Doppler width under 8.3e-4 cm^-1, which H2O has at 200 K only below 700 cm^-1: the 0.5 and 20 cm^-1 tiles
    # sit at 520-541 cm^-1 (cte = 1340, d cte up to 2.6e4); the 2000 cm^-1 tiles end at 2500 and 6000 cm^-1 (cte = 280 and
    # 116) where d cte = 5.5e5 and 2.3e5 is the largest of all -- the one-FMA form's error is 1.2e-7 of that
    T_b, p_b = 200.0, (0.03, 0.005)

    def sampled(v, g, n_coarse, x0, x1):
        cte, _ = _cte_y(v, g, T_b, p_b[0])
        f = v + (np.arange(-16, 17) + 0.31) * 0.25 / cte
        t = np.concatenate([np.linspace(x0, x1, n_coarse - f.size), f])
        assert np.unique(t).size == n_coarse
        return np.sort(t)

    # (centre, gamma_air): y = gamma p cte (Tref/T)^0.7; 2.9-3.7 at 0.03 atm, 0.49-0.62 at 0.005 atm
    b_lines = [(500.0008, 0.07), (520.08, 0.07), (540.5, 0.07), (2500.3, 0.35), (6000.3, 0.8)]
    tiles = [np.full(1024, 500.0), sampled(520.08, 0.07, 1024, 519.6, 520.1), sampled(540.5, 0.07, 1024, 521.0, 541.0),
             sampled(2500.3, 0.35, 1024, 545.0, 2545.0), sampled(6000.3, 0.8, 1024, 4002.0, 6002.0)]
    C["b_span"] = _case(table([v for v, _ in b_lines], [g for _, g in b_lines]), np.concatenate(tiles), T_b, p_b,
                        expect=("band_wei32", "band_w64"))
    # repeated points inside a row, astride a row boundary and astride a tile boundary, lines next to each
    X = np.concatenate([wavy(1000.0, 2e-4, 1500), wavy(1000.31, 4e-3, 1100)])
    for i0, i1 in ((29, 31), (100, 102), (63, 64), (1023, 1024), (2047, 2049)):
        X[i0 + 1:i1 + 1] = X[i0]
    nus = [X[30] + 1e-5, X[66] + 3e-5, X[1021] + 7e-5, X[2050] + 1e-4]
    C["b_repeats"] = _case(table(nus, [0.02, 0.07, 0.005, 0.015]), X, (296.0, 250.0), (1.0, 0.05),
                           expect=("band_wei32", "band_series_y6", "far_rational"))

    # c. windows and the band range, by index ---------------------------------------------------------------------------
    # OmegaWing = 0.25 sets every window (hw = 0): edges on multiples of 64 and on 1024 / 2048, an axis point exactly on
    # nu - W (excluded) and on nu + W (included) with both nextafter neighbours of each
    W = 0.25
    nuA = 1001.7 + 1.23e-4
    edge = [nuA - W, np.nextafter(nuA - W, -np.inf), np.nextafter(nuA - W, np.inf),
            nuA + W, np.nextafter(nuA + W, -np.inf), np.nextafter(nuA + W, np.inf)]
    X = np.unique(np.concatenate([wavy(1000.0, 1e-3, 3 * 1024 + 94), edge]))
    mid = lambda i: 0.5 * (X[i - 1] + X[i])  # nu -+ W here: bisect_right = i
    nus = [nuA, mid(640) + W, mid(1024) - W, mid(2048) + W, mid(1536) - W, mid(1024) + W, mid(2048) - W]
    C["c_edges"] = _case(table(nus, np.resize([0.02, 0.006], len(nus))), X, 296.0, 1.0, ow=W, hw=0.0,
                         expect=("lo_row_aligned", "lo_tile_aligned", "hi_row_aligned", "hi_tile_aligned",
                                 "edge_point_excluded", "edge_point_included", "band_wei32", "band_series_y6",
                                 "!band_clamped_lo"))
    # OmegaWing = 8e-4 (hw = 0): windows of a few points, narrower than the band (clamped to the window on both sides): both
    # edges in one row (fine 1e-4 steps: 16 points), one point, and none at all (a gap of 3e-3 between two points)
    X = np.concatenate([wavy(1000.0, 1e-3, 700), wavy(1000.8, 1e-4, 600), wavy(1000.9, 1e-3, 900, amp=0.2)])
    X = X[~((X > 1001.5) & (X < 1001.503))]
    one = 1001.2
    i1 = int(np.searchsorted(X, one))
    nus = [1000.83 + 1.2e-5, 1001.5015, X[i1], X[100] + 2e-4, X[300] + 1e-4]
    C["c_narrow"] = _case(table(nus, 0.01), X, 296.0, 1.0, ow=8e-4, hw=0.0,
                          expect=("one_row", "one_point", "empty_between_points", "band_clamped_lo", "band_clamped_hi",
                                  "centre_on_point"))
    # OmegaWingHW * Gamma0 windows at Tref, 1 atm: a window over the whole axis, centres left and right of the axis with
    # windows reaching in (ic = 0 and ic = nx), bands cut by both axis ends, a centre exactly on an axis point, and a centre
    # in a 0.02 cm^-1 gap of the axis (band +-0.006: no point in it) whose window is not empty
    X = wavy(1000.0, 1e-3, 3000)
    X = X[~((X > 1001.69) & (X < 1001.71))]
    nus = [999.5, X[0] + 0.003, X[1500], 1001.7, 1001.2 + 1.1e-4, X[-1] - 0.003, X[-1] + 0.5]
    C["c_outside"] = _case(table(nus, [0.07, 0.02, 0.02, 0.02, 0.07, 0.02, 0.07]), X, 296.0, 1.0,
                           expect=("covers_axis", "centre_left", "centre_right", "band_cut_by_axis_end", "centre_on_point",
                                   "band_empty", "band_series_y6"))

    # d. candidate ranges -----------------------------------------------------------------------------------------------
    # two densities (0.02 and 5e-4 cm^-1: 40x). Lines in the fine region (windows of +-3.5 cm^-1 are thousands of points
    # there: maxhw), three of them at one nu; lines centred in the coarse tiles; lines left of the axis whose windows
    # (+-10 cm^-1) reach through tile 0 into tile 1
    X = np.unique(np.concatenate([np.arange(995.0, 1002.0, 0.02), np.arange(1002.0, 1003.0, 5e-4) + 1.7e-4,
                                  np.arange(1003.0, 1010.0, 0.02) + 3e-3]))
    nus = [993.0, 994.0, 997.0 + 1e-3, 1002.3, 1002.3, 1002.3, 1002.31, 1002.7, 1008.0 + 1e-3]
    C["d_two_density"] = _case(table(nus, [0.2, 0.2, 0.07, 0.07, 0.02, 0.11, 0.07, 0.07, 0.07]), X, (296.0, 250.0), (1.0, 0.05),
                               expect=("same_nu", "left_reaches_tile1", "centre_left", "maxhw_layers_differ", "band_wei32"))
    # tiles with 1, 0, 2, 3, 0 and 5 candidates (OmegaWing = 0.05: +-50 points, centres mid-tile)
    X = wavy(1000.0, 1e-3, 6 * 1024)
    at = lambda t, f: X[t * 1024 + int(1024 * f)] + 2.3e-4
    nus = [at(0, 0.5), at(2, 0.4), at(2, 0.6), at(3, 0.3), at(3, 0.5), at(3, 0.7)] + [at(5, f) for f in (0.2, 0.35, 0.5, 0.65, 0.8)]
    C["d_sparse"] = _case(table(nus, np.resize([0.02, 0.009, 0.015], len(nus))), X, 296.0, 1.0, ow=0.05, hw=0.0,
                          expect=("cand_0", "cand_1", "cand_2", "cand_3", "cand_5", "idle_waves", "cand_not_mult4",
                                  "tile_zero_between"))
    # the comb of linesum_cases.c_comb on a perturbed axis: ~600 candidates per tile, every wave takes many slots
    i = np.arange(6 * 1024)
    X = 1000.0 + 1e-3 * (i + 0.3 * np.sin(1.7 * i))
    C["d_comb"] = _case(LC.CASES["c_comb"]["tbl"], X, 296.0, 1.0, expect=("cand_ge_256", "cand_not_mult4"))
    # 1 atm and 1e-4 atm in one call: maxhw is per layer (thousands of points / a few hundred), ic is shared
    nus = np.array([1000.3, 1000.9, 1001.5]) + 1.23e-4
    X = axis(1000.0, 1002.0, 2e-3, [(v, 0.012, 2e-5) for v in nus])
    C["d_layers"] = _case(table(nus), X, 296.0, (1.0, 1e-4), expect=("maxhw_layers_differ", "band_w64", "far_rational"))
    return C


CASES = _cases()
PATH_CASES = sorted(CASES)
# e. the uniform cases of linesum_cases (a-d) on their shard axes, through the axis path
UNIFORM_CASES = {name: _case(c["tbl"], grid_axis(c["grid"]), c["T"], c["p"], c["ow"], c["hw"], uniform=True)
                 for name, c in LC.CASES.items() if name in LC.PATH_CASES}
SHAPES_CASE = "b_repeats"  # X[:n] of it: lines at points 30, 66, 1021 and 2050


def layer_diluent(case, k):
    """The oracle's Diluent of layer k (None: air)."""
    d = case["diluent"]
    return None if d is None else {n: float(np.broadcast_to(v, case["T"].shape)[k]) for n, v in d.items()}


def oracle_fn(case):
    """(function of cpu_ref, extra keyword arguments) for the case's profile."""
    if case["profile"] == 1:
        return cpu_ref.absorptionCoefficient_Lorentz, {}
    if case["profile"] == 2:
        return cpu_ref.absorptionCoefficient_Doppler, {"LineShift": case["lineshift"]}
    return cpu_ref.absorptionCoefficient_Voigt, {}


def oracle(case, X=None, tbl=None, layers=None):
    """[layers][points] of the fp64 oracle on the case's axis (or X), for the case's table (or tbl)."""
    X = case["X"] if X is None else X
    fn, kw = oracle_fn(case)
    out = []
    for k in (range(case["T"].size) if layers is None else layers):
        d = layer_diluent(case, k)
        out.append(fn(case["tbl"] if tbl is None else tbl, T=float(case["T"][k]), p=float(case["p"][k]), OmegaGrid=X,
                      OmegaWing=case["ow"], OmegaWingHW=case["hw"], **({"Diluent": d} if d else {}), **kw)[1])
    return np.stack(out)
