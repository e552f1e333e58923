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


# ---- the fit's linear operator: truth_operator_mp / truth_adjoint_mp ----

def _operator_batch(dim):
    """_benign plus one case that mixes a known derivative with a stray high bit (a known, a dropped DOF and unknowns in one case)."""
    b = _benign(dim, n=14)
    no = b["no"]
    b["kn"][12] = 2 | (1 << (no + 1))
    b["order_a"][12] = 2
    op = P.truth_operator_mp(dim, b["xk"], b["nk"], b["xi"], b["order_a"], b["kn"], b["wm"], as_mp=True)
    return b, op


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_truth_operator_mp_is_the_fit(dim):
    """(i) linearity: S fk + J fi_known is truth_fit_mp's solution to 1e-50; (iii) kappa is truth_fit_mp's; the masks say what the fit
    defines; the float64 form is the rounded mpf form."""
    import mpmath
    b, op = _operator_batch(dim)
    S, J, kappa = op[:3]
    args = (dim, b["xk"], b["fk"], b["nk"], b["xi"], b["fi0"], b["order_a"], b["kn"], b["wm"])
    fit, kappa_fit = P.truth_fit_mp(*args, as_mp=True)
    assert np.array_equal(kappa, kappa_fit)
    seen = set()
    with mpmath.mp.workdps(60):
        for j in range(b["n"]):
            nkj = int(b["nk"][j])
            kind = op.kind[j]
            seen |= set(kind.tolist())
            for a in range(b["no"]):
                if kind[a] != P.DOF_UNKNOWN:
                    assert not op.live[j, :, a].any() and all(S[j, k, a] == 0 for k in range(S.shape[1]))
                    assert all(J[j, a, c] == 0 for c in range(b["no"]))
                    continue
                assert op.live[j, :nkj, a].all() and not op.live[j, nkj:, a].any()
                assert all(J[j, a, c] == 0 for c in range(b["no"]) if kind[c] != P.DOF_KNOWN)
                got = mpmath.fsum(S[j, k, a] * mpmath.mpf(float(b["fk"][j, k])) for k in range(nkj))
                got += mpmath.fsum(J[j, a, c] * mpmath.mpf(float(b["fi0"][j, c])) for c in range(b["no"]))
                assert abs(got - fit[j, a]) <= mpmath.mpf(10) ** -50 * abs(fit[j, a]), (j, a, got, fit[j, a])
    assert seen == {P.DOF_UNKNOWN, P.DOF_KNOWN, P.DOF_DROPPED, P.DOF_BEYOND}
    as64 = P.truth_operator_mp(dim, b["xk"][:3], b["nk"][:3], b["xi"][:3], b["order_a"][:3], b["kn"][:3], b["wm"][:3])
    assert np.array_equal(as64.S, S[:3].astype(np.float64)) and np.array_equal(as64.J, J[:3].astype(np.float64))


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_truth_operator_mp_reproduces_the_monomials(dim):
    """(ii) sum_k S[k, a] c_k[b] = delta_ab over the unknowns, to 1e-50, with the monomials c_k built here from the coordinates: the one
    identity that does not go through the elimination whose result it checks."""
    import mpmath
    from mpmath import mpf
    b, op = _operator_batch(dim)
    fact = [1, 1, 2, 6, 24]
    checked = 0
    with mpmath.mp.workdps(60):
        for j in range(b["n"]):
            ex = P.exponents(dim, int(b["order_a"][j]))
            U = [a for a in range(len(ex)) if op.kind[j, a] == P.DOF_UNKNOWN]
            nkj = int(b["nk"][j])
            c = []
            for k in range(nkj):
                xkj = [b["xk"][j, k]] if dim == 1 else b["xk"][j, k]
                xij = [b["xi"][j]] if dim == 1 else b["xi"][j]
                d = [mpf(float(p)) - mpf(float(q)) for p, q in zip(xkj, xij)]
                c.append([mpmath.fprod(d[m] ** p / fact[p] for m, p in enumerate(e)) for e in ex])
            for a in U:
                for bb in U:
                    got = mpmath.fsum(op.S[j, k, a] * c[k][bb] for k in range(nkj))
                    assert abs(got - (1 if a == bb else 0)) <= mpf(10) ** -50, (j, a, bb, got)
                    checked += 1
    assert checked >= 100 if dim > 1 else checked >= 30


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_truth_adjoint_mp_is_the_transpose(dim):
    """<g, fit(fk, fi)> over the unknowns plus the pass-through of every other DOF = <grad_fk, fk> + <grad_fi, fi>, to fp64 rounding of
    the rounded gradients; padding, unknowns and columns beyond the order are exact zeros; dropped DOFs pass g through; s is the scale
    of tests/_adjoint_ref.contract evaluated on the rounded sensitivities."""
    b, op = _operator_batch(dim)
    n, no = b["n"], b["no"]
    g = np.random.default_rng(40 + dim).uniform(-1, 1, (n, no))
    gfk, gfi, s = P.truth_adjoint_mp(op, g)
    fit, _ = P.truth_fit_mp(dim, b["xk"], b["fk"], b["nk"], b["xi"], b["fi0"], b["order_a"], b["kn"], b["wm"])
    S64 = op.S.astype(np.float64)
    for j in range(n):
        kind = op.kind[j]
        nkj = int(b["nk"][j])
        assert np.all(gfk[j, nkj:] == 0.0)
        assert np.all(gfi[j, (kind == P.DOF_UNKNOWN) | (kind == P.DOF_BEYOND)] == 0.0)
        assert np.array_equal(gfi[j, kind == P.DOF_DROPPED], g[j, kind == P.DOF_DROPPED])
        defined = kind != P.DOF_BEYOND
        lhs = float(np.dot(g[j, defined], fit[j, defined]))
        terms = np.concatenate([gfk[j] * b["fk"][j], gfi[j] * b["fi0"][j]])
        assert abs(lhs - terms.sum()) <= 64 * np.finfo(float).eps * np.abs(terms).sum(), (j, lhs, terms.sum())
        U = kind == P.DOF_UNKNOWN
        want_s = np.abs(S64[j][:, U] * g[j, U]).sum(axis=1).max() if U.any() else 0.0
        assert abs(s[j] - (want_s if want_s > 0 else 1.0)) <= 1e-14 * s[j]
