"""The pointwise metric of the line-sum path suites (tests/test_gpu_linesum_paths.py, tests/test_gpu_linesum_axis_paths.py)
and its floor share (tests/test_linesum_axis_host.py). Per layer:

    err_i = |got_i - want_i| / max(|want_i|, F max_{|j - i| <= HALO} |want_j|, F32_FLOOR)

The floor is local, not global: a far wing, a weak band or a thin layer is held to its own neighbourhood (HALO points to
either side, in index space), not to the strongest layer's peak. Points where the oracle is exactly 0 (outside every window)
must be exactly 0. F32_FLOOR: values fp32 cannot hold are compared absolutely."""
import numpy as np

TOL = 1e-5
F = 1e-5
HALO = 1024
F32_FLOOR = 1e-36  # below fp32's normal range (1.2e-38) with a margin: compared absolutely


def _local_max(a, h=HALO):
    """max |a_j| over |j - i| <= h, per row (doubling: max over [i, i + 2^k) from max over [i, i + 2^(k-1)))."""
    a = np.abs(a)
    n = a.shape[-1]
    pad = np.full(a.shape[:-1] + (h,), 0.0)
    b = np.concatenate([pad, a, pad], axis=-1)  # b[i + h] = a[i]
    m, w = b.copy(), 1
    while 2 * w <= h:
        m[..., :-w] = np.maximum(m[..., :-w], m[..., w:])
        w *= 2
    # m[i] = max b[i, i + w); cover [i, i + 2h] with windows of length w
    out = np.zeros_like(a)
    for s in range(0, 2 * h + 1, w):
        s = min(s, 2 * h + 1 - w)
        out = np.maximum(out, m[..., s:s + n])
    return out


def pointwise_err(got, want):
    """The metric over [layers][points]; inf if a structural zero of the oracle is not exactly 0."""
    got = np.atleast_2d(np.asarray(got, dtype=np.float64))
    want = np.atleast_2d(np.asarray(want, dtype=np.float64))
    assert got.shape == want.shape, (got.shape, want.shape)
    zero = want == 0.0
    if np.any(got[zero] != 0.0):
        return float("inf")
    den = np.maximum(np.maximum(np.abs(want), F * _local_max(want)), F32_FLOOR)
    e = np.abs(got - want) / den
    e[zero] = 0.0
    return float(np.max(e)) if e.size else 0.0


def on_floor(want):
    """bool [layers][points]: the metric's denominator at this point is the floor, not |want| (structural zeros are not
    counted: they are compared exactly)."""
    want = np.atleast_2d(np.asarray(want, dtype=np.float64))
    return (want != 0.0) & (np.abs(want) < np.maximum(F * _local_max(want), F32_FLOOR))
