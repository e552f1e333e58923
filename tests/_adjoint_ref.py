"""Reference answer of the fit's adjoint (wlsqm.hip.fit_many_adjoint_device) built from the CPU oracle, numpy only.

The fit is linear in fk and in the known entries of fi, so its transpose applied to g = dL/dfi_out is
    grad_fk[j, k] = sum_a sens[j, k, a] g[j, a]       over the unknown DOFs a (sens: the fit's sensitivities, NaN / never written elsewhere),
    grad_fi[j, a] = sum_b g[j, b] J[j, b, a],          J[:, :, a] = the fit of fk = 0 from fi = e_a (exact linearity: one oracle fit per DOF).
The two constructions share nothing but the oracle; tests/test_adjoint_cpu.py checks them against each other through the identity
grad_fi[a] = g[a] - sum_k c_k[a] grad_fk[k] that the kernel uses for the known columns."""
import numpy as np

import _cases as K
import _parity as P
from oracle import oracle

UNTOUCHED = 777.0        # what tests/golden/make_golden.py pre-fills sens with


def covered(dim, order):
    """Shapes the adjoint kernels cover: everything but 3D orders 3 and 4."""
    return not (dim == 3 and order >= 3)


def unknowns(dim, order, knowns):
    """Number of DOFs the fit solves for (stray high mask bits drop unknowns: infra.pyx:119-121)."""
    no = K.NDOF[dim][int(order)]
    return max(no - bin(int(knowns) & ((1 << no) - 1)).count("1") - bin(int(knowns) >> no).count("1"), 0)


def resolvable(dim, order, nk, knowns):
    """Per case: at least unknowns + 2 neighbours (the exclusion the existing suites make), and what those suites skip (nk < no + 2)."""
    n = len(nk)
    ok = np.array([nk[j] >= unknowns(dim, order[j], knowns[j]) + 2 for j in range(n)])
    suite = np.array([nk[j] >= K.NDOF[dim][int(order[j])] + 2 for j in range(n)])
    return ok, suite


def contract(sens, g, nk):
    """(grad_fk (n, K), s (n,)) from sensitivities (n, K, >= no): the columns that are NaN or UNTOUCHED (knowns, dropped DOFs, padding) do not
    take part; s[j] = max_k sum_a |sens[j, k, a] g[j, a]|, the scale of the case (1 where there is nothing to scale)."""
    sens = np.asarray(sens, np.float64)
    no = min(sens.shape[2], g.shape[1])
    t = sens[:, :, :no] * g[:, None, :no]
    dead = np.isnan(sens[:, :, :no]) | (sens[:, :, :no] == UNTOUCHED)
    t = np.where(dead, 0.0, t)
    live = np.arange(sens.shape[1])[None, :] < np.asarray(nk)[:, None]
    gfk = np.where(live, t.sum(axis=2), 0.0)
    s = np.where(live, np.abs(t).sum(axis=2), 0.0).max(axis=1)
    return gfk, np.where(s > 0, s, 1.0)


def adjoint_ref(dim, order, xk, nk, xi, knowns, wm, g, sens=None):
    """order: an int or a per-case int32 array; g (n, >= max no).  Returns dict(grad_fk (n, K), grad_fi (n, max no), s (n,), sens).
    `sens`: use these sensitivities (the real reference's golden ones) instead of the oracle's for grad_fk and s."""
    n = len(nk)
    order = np.full(n, order, np.int32) if np.isscalar(order) else np.asarray(order, np.int32)
    no_max = max(K.NDOF[dim][int(o)] for o in order)
    Kn = xk.shape[1]
    zeros_fk = np.zeros((n, Kn))
    if sens is None:
        sens = np.full((n, Kn, no_max), np.nan)
        fi = np.zeros((n, no_max))
        oracle.fit_many(dim, xk, zeros_fk, nk, xi, fi, sens, 1, order, knowns, wm)
    gfk, s = contract(sens, g, nk)
    gfi = np.zeros((n, no_max))
    with np.errstate(invalid="ignore"):
        for a in range(no_max):
            fi = np.zeros((n, no_max)); fi[:, a] = 1.0
            oracle.fit_many(dim, xk, zeros_fk, nk, xi, fi, None, 0, order, knowns, wm)
            for j in range(n):
                no = K.NDOF[dim][int(order[j])]
                if a < no:
                    gfi[j, a] = float(np.dot(g[j, :no], fi[j, :no]))
    return dict(grad_fk=gfk, grad_fi=gfi, s=s, sens=sens)


def monomial_sums(dim, order, xk, nk, xi, gfk):
    """sum_k c_k[a] gfk[j, k] per case and DOF, c_k the scaled monomials of neighbour k (numpy, independent of the oracle)."""
    n = len(nk)
    order = np.full(n, order, np.int32) if np.isscalar(order) else np.asarray(order, np.int32)
    no_max = max(K.NDOF[dim][int(o)] for o in order)
    out = np.zeros((n, no_max))
    for j in range(n):
        ex = P.exponents(dim, int(order[j]))
        m = int(nk[j])
        d = (xk[j, :m] - xi[j])[:, None] if dim == 1 else xk[j, :m, :dim] - xi[j, None, :dim]
        for a, e in enumerate(ex):
            c = np.ones(m)
            for q, p in enumerate(e):
                if p:
                    c = c * d[:, q] ** p / P._FACT[p]
            out[j, a] = float(np.dot(c, gfk[j, :m]))
    return out


def noise_floor(dim, seed=7):
    """The fp64 noise floor N of grad_fk on the reference sweep of `dim`: per case the distance between the contraction of the ORACLE's
    sensitivities and of the REAL reference's golden ones, over the case's scale; the maximum over the resolvable cases of the shapes
    the adjoint covers.  Returns (N, dict with the pieces the tests share: the sweep, g, the oracle-built reference, the masks)."""
    d = K.sweep(dim)
    n = len(d["nk"])
    cov = np.array([covered(dim, o) for o in d["order"]])
    ok, suite = resolvable(dim, d["order"], d["nk"], d["knowns"])
    no_max = d["fi_in"].shape[1]
    g = np.random.default_rng(seed).uniform(-1.0, 1.0, (n, no_max))
    ref = adjoint_ref(dim, d["order"], d["xk"], d["nk"], d["xi"], d["knowns"], d["wm"], g)
    gold_fk, gold_s = contract(d["sens"], g, d["nk"])
    use = cov & ok
    e = np.abs(ref["grad_fk"] - gold_fk).max(axis=1) / ref["s"]
    N = float(e[use].max())
    return N, dict(d=d, g=g, ref=ref, gold_fk=gold_fk, gold_s=gold_s, use=use, cov=cov, ok=ok, suite=suite, e=e)
