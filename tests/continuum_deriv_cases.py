"""Shared helpers of the continuum-derivative tests (tests/test_continuum_deriv_host.py on the CPU,
tests/test_gpu_continuum_deriv.py on the device); no test in here. The inputs are those of tests/continuum_cases.py."""
import numpy as np

import continuum_cases as K


def stencil_sums(cont, X, T, P, PL, MF, ID):
    """Per component of `cont`, in float64 from the float64 rows A: (S [nL][nX] the stencil sum of the definition,
    M [nL][nX] = sum_k |L_k A_k| its magnitude, inside [nX]); S and M are 0 outside the component's axis."""
    X = np.asarray(X, dtype=np.float64)
    out = []
    for c, A in zip(cont.components, cont.layer_rows(T, P, PL, MF, ID)):
        inside, j0, Lk = c.stencil(X)
        S = np.array([sum(Lk[k] * A[l, j0 + k] for k in range(4)) for l in range(A.shape[0])])
        M = np.array([sum(np.abs(Lk[k] * A[l, j0 + k]) for k in range(4)) for l in range(A.shape[0])])
        out.append((np.where(inside, S, 0.0), np.where(inside, M, 0.0), inside))
    return out


def component_lists(cont_mod, name):
    """The component lists of the kernel tests on grid `name` (continuum_cases.GRIDS): {key: (Continuum, species)} with
    species the molecule ids of K's slots.
      one     one component;
      two     two components on different molecules, two slots;
      shared  two components of one molecule: one slot;
      skip    two components, the second one's molecule not differentiated (slot -1);
      five    five components on two molecules, the slots in the other order: the fifth starts a second register group."""
    (m1, v1, d1, n1, k1), (m2, v2, d2, n2, k2) = K.GRIDS[name]["comps"]
    a = K.component(cont_mod, m1, v1, d1, n1, seed=3, kind=k1)
    b = K.component(cont_mod, m2, v2, d2, n2, seed=4, kind=k2)
    b_on_1 = K.component(cont_mod, m1, v2, d2, n2, seed=4, kind=k2)
    a_self = K.component(cont_mod, m1, v1, d1, n1, seed=8, kind="self")
    a_foreign_2 = K.component(cont_mod, m2, v1, d1, n1, seed=9, kind="foreign")
    return {"one": (a, (m1,)), "two": (a + b, (m1, m2)), "shared": (a + b_on_1, (m1,)), "skip": (a + b, (m1,)),
            "five": (a + b + a_self + a_foreign_2 + b_on_1, (m2, m1))}
