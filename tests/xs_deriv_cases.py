"""Shapes and fixtures of the cross-section-table derivative tests (tests/test_xs_lut_deriv_host.py on the CPU,
tests/test_gpu_xs_lut_deriv.py on the device); no test in here. Host NumPy only.

The random table: molecules 1 and 2 on 3 x 2 (T, p) nodes each, molecule 6 on a single T node with 2 p nodes, on one axis of
N_AXIS points (two tiles of 1024 and a ragged rest, plus room for an offset). The layers: 3 (or the first of them), the
second EXACTLY ON the middle T node of molecules 1 and 2, the others inside a cell."""
import numpy as np

TILE = 1024
N_AXIS = 2 * TILE + 12
N_POINTS = (1, 3, 65, 1024, 1027, 2051)   # one point, a ragged quad, part of a tile, one tile, tile + ragged, two tiles + ragged
OFFSETS = (4, 5)                          # divisible by 4 (16-byte accesses) and not (point by point)
SPECIES_LISTS = ((), (1,), (1, 2), (2, 1))
T_NODES = np.array([230.0, 260.0, 300.0])
P_NODES = np.array([0.2, 1.0])
IDS = np.array([1, 2, 6])


def entries():
    """from_grids entries of the random table (seeded), float64 cross sections between 1e-26 and 1e-19 cm^2."""
    rng = np.random.default_rng(20261020)
    X = np.linspace(2000.0, 2000.0 + 0.01 * (N_AXIS - 1), N_AXIS)
    shapes = ((1, T_NODES, P_NODES), (2, T_NODES, P_NODES), (6, np.array([270.0]), P_NODES))
    return [dict(ID=ID, T=np.array(T), P_atm=np.array(P), X=X, xs=10.0 ** rng.uniform(-26.0, -19.0, (len(T), len(P), N_AXIS)))
            for ID, T, P in shapes]


def tables(ents):
    """layer_terms' `tables` of the entries: [(ID, T_nodes, P_nodes, row0)], and the float64 rows [n_rows][nX]."""
    out, row0, rows = [], 0, []
    for e in ents:
        out.append((int(e["ID"]), np.asarray(e["T"], dtype=np.float64), np.asarray(e["P_atm"], dtype=np.float64), row0))
        row0 += e["T"].size * e["P_atm"].size
        rows.append(np.asarray(e["xs"], dtype=np.float64).reshape(-1, N_AXIS))
    return out, np.concatenate(rows)


def layers(nL):
    """The first nL of three layers: inside a cell; exactly on the middle T node; inside the other cell."""
    assert 1 <= nL <= 3
    rng = np.random.default_rng(7)
    MF = rng.uniform(50.0, 2e4, (3, 3))
    lay = dict(T=np.array([281.3, 260.0, 244.9]), P=np.array([0.47, 0.6, 0.31]), PL=np.array([1.0, 0.5, 2.0]), MF=MF, ID=IDS)
    if nL == 1:  # the single layer is the one on the node
        return {k: (v[1:2] if k != "ID" else v) for k, v in lay.items()}
    return {k: (v[:nL] if k != "ID" else v) for k, v in lay.items()}


def largs(lay):
    return lay["T"], lay["P"], lay["PL"], lay["MF"], lay["ID"]


def forward_od(tabs, xs_rows, T, P, PL, MF, ID):
    """DESIGN 4.11 in float64 from afit_xs.layer_terms' rows and weights: OD[l][x]."""
    from radtxfr_amd import afit_xs
    rows, w = afit_xs.layer_terms(tabs, T, P, PL, MF, ID)
    out = np.zeros((rows.shape[0], xs_rows.shape[1]))
    for l in range(rows.shape[0]):
        for m in range(rows.shape[1]):
            for c in range(4):
                out[l] += w[l, m, c] * xs_rows[rows[l, m, c]]
    return out
