"""A float64 numpy statement of the adjoint of InterpolationPlan.evaluate, and of the forward it is the adjoint of.

Both are fed with the plan's own I (nearest) or lists (continuous), so the search is not under test.  With P the exponent table, c the
scaled monomials of x_m - xi[model] and Q_j = diffs[j]:

    nearest:     grad_fi[i, a] = sum over m with I_m == i, over j with P_a >= P_Qj:   g[j, m] c_m[index(P_a - P_Qj)]        (a < no_i)
    continuous:  grad_fi[i, a] = sum over (m, e) with idx[e] == i, over j as above:   (w_me / W_m) g[j, m] c_me[index(P_a - P_Qj)]

with w_me = (1 - sqrt(d2 / r2))^2 and W_m = sum_e w_me.  Points with I_m outside 0 .. nmodels - 1, with an empty list or with W_m == 0
contribute nothing and their g is not read.  Beside the sums, adjoint() returns per element the sum A of the absolute values of its terms
and their number n, from which the tests size their bounds."""
import numpy as np

NDOF = {1: (1, 2, 3, 4, 5), 2: (1, 3, 6, 10, 15), 3: (1, 4, 10, 20, 35)}
# exponents (p, q, r) of DOF a (wlsqm.fitter.defs: i1_*, i2_*, i3_*)
EXPONENTS = {
    1: [(p, 0, 0) for p in range(5)],
    2: list(zip((0, 1, 0, 2, 1, 0, 3, 2, 1, 0, 4, 3, 2, 1, 0), (0, 0, 1, 0, 1, 2, 0, 1, 2, 3, 0, 1, 2, 3, 4), (0,) * 15)),
    3: list(zip((0, 1, 0, 0, 2, 1, 0, 0, 0, 1, 3, 2, 1, 0, 0, 0, 0, 1, 2, 1, 4, 3, 2, 1, 0, 0, 0, 0, 0, 1, 2, 3, 2, 1, 1),
                (0, 0, 1, 0, 0, 1, 2, 1, 0, 0, 0, 1, 2, 3, 2, 1, 0, 0, 0, 1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 0, 0, 0, 1, 2, 1),
                (0, 0, 0, 1, 0, 0, 0, 1, 2, 1, 0, 0, 0, 0, 1, 2, 3, 2, 1, 1, 0, 0, 0, 0, 0, 1, 2, 3, 4, 3, 2, 1, 1, 1, 2))),
}
FACT = (1.0, 1.0, 2.0, 6.0, 24.0)
EPS = float(np.finfo(np.float64).eps)


def scaled_monomials(dim, dx):
    """c[:, b] = prod_m dx[:, m]^e / e! for the exponents of DOF b."""
    c = np.ones((dx.shape[0], len(EXPONENTS[dim])))
    for b, e in enumerate(EXPONENTS[dim]):
        for m in range(dim):
            c[:, b] *= dx[:, m] ** e[m] / FACT[e[m]]
    return c


def triples(dim, diffs):
    """(j, a, b) for every requested diff j and DOF a with P_a >= P_Qj: b = index(P_a - P_Qj).  A diff outside the table gives none."""
    E = EXPONENTS[dim]
    index = {e: b for b, e in enumerate(E)}
    out = []
    for j, Q in enumerate(diffs):
        if not 0 <= Q < len(E):
            continue
        for a in range(len(E)):
            e = tuple(E[a][m] - E[Q][m] for m in range(3))
            if min(e) >= 0:
                out.append((j, a, index[e]))
    return out


def entries(dim, xi, x, nmodels, I=None, lists=None, r=None):
    """The (point, model, scale) entries that carry a dependence on fi, with their offsets, and the longest list of a contributing
    point (0 in nearest mode).  xi (nmodels, dim), x (nx, dim)."""
    xi, x = np.asarray(xi, float).reshape(-1, dim), np.asarray(x, float).reshape(-1, dim)
    if I is not None:
        I = np.asarray(I)
        pt = np.nonzero((I >= 0) & (I < nmodels))[0]
        model = I[pt]
        return pt, model, np.ones(len(pt)), x[pt] - xi[model], 0
    off, idx = (np.asarray(t) for t in lists)
    nx = len(off) - 1
    length = np.diff(off)
    pt = np.repeat(np.arange(nx), length)
    dx = x[pt] - xi[idx]
    w = (1.0 - np.sqrt((dx * dx).sum(axis=1) / (r * r))) ** 2
    W = np.bincount(pt, weights=w, minlength=nx)
    keep = W[pt] != 0.0
    len_max = int(length[W != 0.0].max()) if (W != 0.0).any() else 0
    return pt[keep], idx[keep], w[keep] / W[pt][keep], dx[keep], len_max


def forward(dim, xi, order, x, fi, diffs, I=None, lists=None, r=None):
    """out[j, m] = d^Qj of the (weighted average of the) models at x_m: 0 where fi does not reach (the device gives NaN at some of
    those points; the dot-product identity does not look there)."""
    nmodels, nx = len(order), np.asarray(x).reshape(-1, dim).shape[0]
    pt, model, scale, dx, _ = entries(dim, xi, x, nmodels, I, lists, r)
    c = scaled_monomials(dim, dx)
    no = np.array(NDOF[dim])[np.asarray(order)][model]
    out = np.zeros((len(diffs), nx))
    for j, a, b in triples(dim, diffs):
        if a >= fi.shape[1]:
            continue
        term = np.where(a < no, scale * fi[model, a] * c[:, b], 0.0)
        out[j] += np.bincount(pt, weights=term, minlength=nx)
    return out


def adjoint(dim, xi, order, x, g, diffs, ncols, I=None, lists=None, r=None):
    """(grad_fi (nmodels, ncols), A, n, len_max): the sums, per element the sum of the absolute values of the terms and their number,
    and the longest list of a contributing point.  g (ndiff, nx); g is read at the contributing entries only."""
    nmodels = len(order)
    g = np.asarray(g, float).reshape(len(diffs), -1)
    pt, model, scale, dx, len_max = entries(dim, xi, x, nmodels, I, lists, r)
    c = scaled_monomials(dim, dx)
    no = np.array(NDOF[dim])[np.asarray(order)][model]
    grad, A, n = np.zeros((nmodels, ncols)), np.zeros((nmodels, ncols)), np.zeros((nmodels, ncols), dtype=np.int64)
    for j, a, b in triples(dim, diffs):
        if a >= ncols:
            continue
        has = a < no
        term = np.where(has, scale * g[j, pt] * c[:, b], 0.0)
        grad[:, a] += np.bincount(model, weights=term, minlength=nmodels)
        A[:, a] += np.bincount(model, weights=np.abs(term), minlength=nmodels)
        n[:, a] += np.bincount(model, weights=has, minlength=nmodels).astype(np.int64)
    return grad, A, n, len_max


def bound(A, n, len_max):
    """|got - ref| <= (128 + 4 (n + len_max)) eps A per element: each term carries a handful of roundings (monomial, weight, w / W),
    W is a sum of at most len_max terms, and a sum of n terms adds n eps in any order (the butterfly of the wave form included)."""
    return (128.0 + 4.0 * (n + len_max)) * EPS * A
