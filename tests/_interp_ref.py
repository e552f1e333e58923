"""ExpertSolver.interpolate and InterpolationPlan.evaluate stated in numpy long double (x87, eps 5.4e-20), the fp64 replay of the
kernels' arithmetic that tests/test_interp_ref_host.py measures the bounds on, and the geometry both test modules use.

The model of origin xi, order o and coefficients f, differentiated by the multi-index Q = exponents[diff], at x:
    sum over the DOFs a < no(o) with P_a >= Q of  f[a] prod_m (x_m - xi_m)^(P_a - Q)_m / (P_a - Q)_m!
(exponent tables: _parity.exponents); a diff the model does not have contributes 0.  mode='nearest' is the value of model I[m];
mode='continuous' is sum_i w_i v_i / sum_i w_i over the models within r, w = (1 - sqrt(d2 / r^2))^2, NaN on an empty list.

Bounds (T = sum over the surviving terms of |f[a]| |monomial|, in fp64):
  nearest      64 eps T_m: at most 35 terms of at most 3 roundings each and the running sum; half of the two-implementation bound of
               tests/test_gpu_interp_plan.py, because the truth is exact.
  continuous   eps ((64 + 4 len) sum_i w_i T_i + 16 sum_i T_i) / sum_i w_i: the same per model plus the weighted sums over the list; the
               second term is the absolute rounding of a weight (sqrt, quotient and difference of numbers near 1: about 2 eps on
               t = 1 - sqrt(d2 / r^2), so 4 eps t <= 4 eps on w = t^2), which enters once through the numerator and once through the
               denominator and does not shrink with the weight: for a point just inside a sphere it is all there is.
The host test replays both in fp64 and prints the largest ratio to these bounds per dimension; neither passes 0.5."""
import numpy as np

import _parity as P

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
NDOF = P._NDOF
NMODELS = 1500
NX = 5 * 64 + 17                   # 337: five full waves and a partial one
NEAR_SPHERE = 24                   # of them, just inside the sphere of a model
TOP = {1: 4, 2: 4, 3: 3}           # orders mixed over 0..top (3D: 30 neighbours do not carry the 35 unknowns of order 4)
NEIGHBOURS = {1: 8, 2: 24, 3: 30}
RADIUS = {1: 0.004, 2: 0.05, 3: 0.15}


def _rows(dim, a):
    a = np.asarray(a)
    return a.reshape(-1, dim) if a.ndim == 1 else a[:, :dim]


def _csr(lists, nx):
    length = np.array([len(L) for L in lists], np.int64)
    assert len(length) == nx
    idx = np.array([i for L in lists for i in L], np.int64)
    return np.repeat(np.arange(nx), length), idx, length


def _values(dim, xi, fi, order, models, pts, diff):
    """Long double: the `diff` derivative of model models[e] at pts[e], and the squared distance to its origin, per entry e."""
    E = P.exponents(dim, 4)
    dx = np.asarray(pts, LD) - np.asarray(xi, LD)[models]
    d2 = (dx * dx).sum(axis=1)
    acc = np.zeros(len(models), LD)
    if not 0 <= diff < len(E):
        return acc, d2
    no = np.asarray(NDOF[dim])[np.asarray(order)[models]]
    for a, e in enumerate(E[:fi.shape[1]]):
        left = tuple(e[m] - E[diff][m] for m in range(dim))
        if min(left) < 0:
            continue
        term = np.asarray(fi[models, a], LD)
        for m, p in enumerate(left):
            if p:
                term = term * dx[:, m] ** p / LD(P._FACT[p])
        acc = acc + np.where(a < no, term, LD(0))
    return acc, d2


def truth_interpolate(dim, xi, fi, order, x, diff, I=None, lists=None, r=None):
    """interpolate() in long double.  xi (n, dim) [1D: (n,)], fi (n, >= max_no), order (n,), x (nx, dim) [1D: (nx,)].  With I (nx,): the
    value of model I[m] (NaN where I[m] is no model).  With lists (nx lists of model indices) and r: the weighted average, NaN on an
    empty list.  Returns long double (nx,)."""
    xi, x = _rows(dim, xi), _rows(dim, x)
    nx = x.shape[0]
    if lists is None:
        I = np.asarray(I, np.int64)
        ok = (I >= 0) & (I < xi.shape[0])
        out = np.full(nx, np.nan, LD)
        out[ok] = _values(dim, xi, fi, order, I[ok], x[ok], diff)[0]
        return out
    pt, idx, _ = _csr(lists, nx)
    v, d2 = _values(dim, xi, fi, order, idx, x[pt], diff)
    t = LD(1) - np.sqrt(d2 / (LD(r) * LD(r)))
    w = t * t
    acc, sum_w = np.zeros(nx, LD), np.zeros(nx, LD)
    np.add.at(acc, pt, w * v)
    np.add.at(sum_w, pt, w)
    with np.errstate(invalid="ignore"):
        return acc / sum_w


def term_sum(dim, xi, fi, order, models, pts, diff):
    """T per entry: sum over the terms that survive `diff` of |fi[model, a]| |monomial_a(pts - xi[model])| (fp64)."""
    E = P.exponents(dim, 4)
    T = np.zeros(len(models))
    if not 0 <= diff < len(E):
        return T
    dx = np.abs(pts - xi[models])
    no = np.asarray(NDOF[dim])[np.asarray(order)[models]]
    for a, e in enumerate(E[:fi.shape[1]]):
        left = tuple(e[m] - E[diff][m] for m in range(dim))
        if min(left) < 0:
            continue
        term = np.abs(fi[models, a])
        for m, p in enumerate(left):
            if p:
                term = term * dx[:, m] ** p / P._FACT[p]
        T += np.where(a < no, term, 0.0)
    return T


def nearest_bound(dim, xi, fi, order, x, diff, I):
    xi, x = _rows(dim, xi), _rows(dim, x)
    return 64 * EPS * term_sum(dim, xi, fi, order, np.asarray(I, np.int64), x, diff)


def continuous_bound(dim, xi, fi, order, x, diff, lists, r):
    """The bound per point (0 for an empty list, where the value is NaN)."""
    xi, x = _rows(dim, xi), _rows(dim, x)
    nx = x.shape[0]
    pt, idx, length = _csr(lists, nx)
    T = term_sum(dim, xi, fi, order, idx, x[pt], diff)
    dx = x[pt] - xi[idx]
    w = (1.0 - np.sqrt((dx * dx).sum(axis=1) / (r * r))) ** 2
    swT, sT, sw = (np.bincount(pt, weights=v, minlength=nx) for v in (w * T, T, w))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(length > 0, EPS * ((64 + 4 * length) * swT + 16 * sT) / sw, 0.0)


def _replay_values(dim, xi, fi, order, models, pts, diff):
    """fp64, operation by operation as eval_model (csrc/wlsqm_interp.hpp): the scaled powers, the products, the running sum."""
    E = P.exponents(dim, 4)
    d = pts - xi[models]
    d2 = np.zeros(len(models))
    for m in range(dim):
        d2 = d2 + d[:, m] * d[:, m]
    acc = np.zeros(len(models))
    if not 0 <= diff < len(E):
        return acc, d2
    pw = [[np.ones(len(models)), d[:, m], 0.5 * d[:, m] * d[:, m], (1.0 / 6.0) * d[:, m] * d[:, m] * d[:, m],
           (1.0 / 24.0) * (d[:, m] * d[:, m]) * (d[:, m] * d[:, m])] for m in range(dim)]
    no = np.asarray(NDOF[dim])[np.asarray(order)[models]]
    for a, e in enumerate(E[:fi.shape[1]]):
        left = tuple(e[m] - E[diff][m] for m in range(dim))
        if min(left) < 0:
            continue
        term = fi[models, a] * pw[0][left[0]]
        for m in range(1, dim):
            term = term * pw[m][left[m]]
        acc = acc + np.where(a < no, term, 0.0)
    return acc, d2


def replay_interpolate(dim, xi, fi, order, x, diff, I=None, lists=None, r=None):
    """The kernels' arithmetic in numpy fp64 (interp_kernel / interp_ball_kernel): what an fp64 implementation of these formulas gives."""
    xi, x = _rows(dim, xi), _rows(dim, x)
    nx = x.shape[0]
    if lists is None:
        return _replay_values(dim, xi, fi, order, np.asarray(I, np.int64), x, diff)[0]
    pt, idx, _ = _csr(lists, nx)
    v, d2 = _replay_values(dim, xi, fi, order, idx, x[pt], diff)
    t = 1.0 - np.sqrt(d2 / (r * r))
    w = t * t
    acc, sum_w = np.zeros(nx), np.zeros(nx)
    np.add.at(acc, pt, w * v)                                   # unbuffered: entry by entry, the lanes' order
    np.add.at(sum_w, pt, w)
    with np.errstate(invalid="ignore"):
        return acc / sum_w


# ------------------------------------------------------------------------------------------------------------------------ geometry
_GEOMETRY = {}


def geometry(dim):
    """The cloud, its neighbourhoods, per-model orders, query points, their nearest models and balls, and one random coefficient array.
    NMODELS models uniform in the unit box; NX query points in [-0.2, 1.2]^dim, so that some lie outside the cloud and some have empty
    balls; the last NEAR_SPHERE of them sit just inside the sphere of radius r around a model, at r (1 - 10^-u), u in [3, 9].  Built
    once, never modified."""
    if dim in _GEOMETRY:
        return _GEOMETRY[dim]
    import scipy.spatial
    n, k, top, r = NMODELS, NEIGHBOURS[dim], TOP[dim], RADIUS[dim]
    rng = np.random.default_rng(50 + dim)
    S = rng.uniform(0.0, 1.0, size=(n, dim))
    F = np.sin(2.0 * S).prod(axis=1)
    tree = scipy.spatial.cKDTree(S)
    hoods = tree.query(S, k + 1)[1][:, 1:]
    order = rng.integers(0, top + 1, size=n).astype(np.int32)
    max_no = NDOF[dim][top]
    X = rng.uniform(-0.2, 1.2, size=(NX, dim))
    centre = rng.integers(0, n, NEAR_SPHERE)
    u = rng.standard_normal((NEAR_SPHERE, dim))
    u /= np.sqrt((u * u).sum(axis=1))[:, None]
    X[NX - NEAR_SPHERE:] = S[centre] + r * (1.0 - 10.0 ** -rng.uniform(3.0, 9.0, (NEAR_SPHERE, 1))) * u
    d2 = ((X[:, None, :] - S[None, :, :]) ** 2).sum(axis=2)      # brute force: (NX, n)
    nearest = d2.argmin(axis=1)
    two = np.partition(d2, 1, axis=1)[:, :2]
    lists = scipy.spatial.cKDTree(X).query_ball_tree(tree, r=r)
    # points with an origin within 1e-12 r of the sphere may fall either way
    edge = tree.query_ball_point(X, r * (1 + 1e-12), return_length=True) != tree.query_ball_point(X, r * (1 - 1e-12), return_length=True)
    given = nearest.copy()                                      # I=: the nearest model for every other point, any model for the rest
    given[1::2] = rng.integers(0, n, len(given[1::2]))
    g = dict(dim=dim, n=n, k=k, r=r, S=S, F=F, hoods=hoods, order=order, no=np.asarray(NDOF[dim])[order], max_no=max_no, X=X,
             xi=S[:, 0].copy() if dim == 1 else S, xk=S[hoods][:, :, 0].copy() if dim == 1 else S[hoods],
             xq=X[:, 0].copy() if dim == 1 else X, nearest=nearest, nearest_gap=(two[:, 1] - two[:, 0]) / two[:, 1], lists=lists,
             edge=edge, empty=np.array([len(L) == 0 for L in lists]), given=given, centre=centre,
             fi_random=rng.standard_normal((n, max_no)))
    for v in g.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _GEOMETRY[dim] = g
    return g
