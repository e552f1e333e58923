"""CPU pins of `_parity.truth_fit_mp`, the mpmath truth the adversarial tests are measured against: it agrees with the x87 truth
where that one is a truth, and it recovers a polynomial exactly where every input is a dyadic rational."""
import numpy as np
import pytest

import _adversarial as A
import _parity as P


def _benign(dim, n=12):
    """Order 2 on twice the unknowns' worth of neighbours, every feature truth_fit handles: ragged nk, knowns masks (none, F, one
    derivative, everything, a stray bit beyond the DOFs), both weightings, per-case orders, the 1D layout."""
    order, K = 2, {1: 8, 2: 16, 3: 24}[dim]
    b = A.make("plain", dim, order, K, n)
    rng = np.random.default_rng(dim)
    no = b["no"]
    b["nk"] = rng.integers(K - 3, K + 1, n).astype(np.int32)
    b["order_a"] = np.where(np.arange(n) % 3 == 2, 1, 2).astype(np.int32)
    b["kn"] = np.array([0, 1, 2, 1 | (1 << (no - 1)), (1 << no) - 1, 1 << (no + 1)], np.int64)[np.arange(n) % 6]
    b["wm"] = np.where(np.arange(n) % 2, 1, 2).astype(np.int32)
    return b


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_truth_fit_mp_equals_truth_fit_on_a_benign_batch(dim):
    b = _benign(dim)
    args = (dim, b["xk"], b["fk"], b["nk"], b["xi"], b["fi0"], b["order_a"], b["kn"], b["wm"])
    got, kappa = P.truth_fit_mp(*args)
    want = P.truth_fit(*args)
    assert got.shape == want.shape and kappa.shape == (b["n"],)
    rel = np.abs(got - want) / np.abs(want).max(axis=0)
    assert rel.max() <= 1e-15, rel.max(axis=0)
    assert np.all(kappa >= 1.0) and np.all(kappa < 1e3), kappa
    solved = np.array([bin(~int(k) & ((1 << A.NDOF[dim][int(o)]) - 1)).count("1") - bin(int(k) >> A.NDOF[dim][int(o)]).count("1") > 0
                       for k, o in zip(b["kn"], b["order_a"])])
    assert np.all(kappa[~solved] == 1.0)
    for j in range(b["n"]):                                     # known DOFs, dropped unknowns and columns beyond the case's order: untouched
        no = A.NDOF[dim][int(b["order_a"][j])]
        kn = int(b["kn"][j])
        for a in range(b["no"]):
            if a >= no or (kn >> a) & 1:
                assert got[j, a] == b["fi0"][j, a]


@pytest.mark.parametrize("dim,order,K", [(1, 4, 12), (2, 2, 32), (2, 4, 64), (3, 3, 64)])
@pytest.mark.parametrize("wm", [1, 2])
def test_truth_fit_mp_recovers_a_dyadic_polynomial(dim, order, K, wm):
    """Lattice offsets and dyadic coefficients: every input is exact, the field IS the model, so the fit returns the coefficients to
    the working precision (60 digits; the weights' square roots are the only inexact operations)."""
    n = 4
    b = A.make("exactpoly_grid", dim, order, K, n)
    kn = np.array([0, 1, 0, 2], np.int64)
    fi0 = b["fi0"].copy()
    fi0[:, :2] = b["coef"][:, :2]                                # the known values are the true ones
    got, kappa = P.truth_fit_mp(dim, b["xk"], b["fk"], b["nk"], b["xi"], fi0, b["order_a"], kn, np.full(n, wm, np.int32), as_mp=True)
    import mpmath
    with mpmath.mp.workdps(60):
        err = max(abs(got[j, a] - mpmath.mpf(float(b["coef"][j, a]))) for j in range(n) for a in range(b["no"]))
        assert err <= mpmath.mpf(10) ** -40, err
