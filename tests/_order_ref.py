"""The Morton order of a cloud, stated once in numpy (wlsqm.hip.SpatialOrder, csrc/order.hip).  The device must
reproduce every function here bit for bit.

Input: S (npoints, dim) float64, dim 1..3, or (npoints,) for 1D; finite coordinates in the domain of knn.  Per axis lo = min, hi = max
over the points, ext = hi - lo (one rounded subtraction).

dim 2 and 3.  B = 31 (2D) or 21 (3D) bits per axis; q = 0 where ext == 0, else q = min(floor(((x - lo) / ext) * 2^B), 2^B - 1): one
correctly rounded subtraction, one correctly rounded division and an exact scaling (no product is followed by a sum: nothing can be
contracted).  Bit b of axis m is bit b * dim + m of the key, as in synth.morton_order; keys are non-negative int64, 62 or 63 bits.
dim 1.  Exact: u = bits(x + 0.0) as int64 (-0.0 becomes +0.0); key = u where u >= 0, else u ^ 0x7fffffffffffffff.

perm is the stable ascending sort of the keys (ties go to the smaller old index): new position i holds old point perm[i], and
inverse[perm[i]] = i.

keys() also places points that are not the cloud's under a given box: outside it they clamp to its ends, and a NaN coordinate gives the
largest key of the dimension.

Lattice clouds (lattice): origin + J * 2^s with integer J in 0 .. 2^p and both corners present have q = J << (B - p) exactly, clamped
at the upper face — an integer truth in the style of tests/_search_cases.py."""
import numpy as np

BITS = {1: 64, 2: 31, 3: 21}
LARGEST = {1: 2 ** 63 - 1, 2: 2 ** 62 - 1, 3: 2 ** 63 - 1}

# the lattice clouds of the tests: origins and shifts (coordinates origin + J * 2^s)
ORIGINS = (0.0, 1e6, -3.0, 2.0 ** 100)
SHIFTS = (-400, -60, -3, 0, 7, 60)


def as_points(S):
    S = np.asarray(S, np.float64)
    return S[:, None] if S.ndim == 1 else S


def box(S):
    S = as_points(S)
    return S.min(axis=0), S.max(axis=0)


def cells(X, lo, hi, B):
    """q (n, dim) int64 of the points X under the box lo .. hi: the statement, with the clamps of a point outside the box."""
    X = as_points(X)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = hi - lo
    q = np.zeros(X.shape, np.int64)
    with np.errstate(all="ignore"):
        for m in range(X.shape[1]):
            if not ext[m] > 0.0:
                continue
            d = X[:, m] - lo[m]
            t = d / ext[m]
            u = t * 2.0 ** B
            inside = (u > 0.0) & (u < 2.0 ** B)
            q[:, m] = np.where(u >= 2.0 ** B, 2 ** B - 1, np.where(inside, np.floor(np.where(inside, u, 0.0)), 0.0).astype(np.int64))
    return q


def interleave(q, B):
    """Bit b of axis m of q (n, dim) is bit b * dim + m of the key."""
    dim = q.shape[1]
    key = np.zeros(q.shape[0], np.int64)
    for b in range(B):
        for m in range(dim):
            key |= ((q[:, m] >> b) & 1) << (b * dim + m)
    return key


def keys1(x):
    u = (np.asarray(x, np.float64) + 0.0).view(np.int64)
    return np.where(u >= 0, u, u ^ np.int64(0x7fffffffffffffff))


def keys(X, lo=None, hi=None):
    """int64 keys of the points X under the box lo .. hi (default: X's own)."""
    X = as_points(X)
    dim = X.shape[1]
    if lo is None:
        lo, hi = box(X)
    lo, hi = np.atleast_1d(np.asarray(lo, np.float64)), np.atleast_1d(np.asarray(hi, np.float64))
    nan = np.isnan(X).any(axis=1)
    if dim == 1:
        k = keys1(np.clip(np.where(nan, lo[0], X[:, 0]), lo[0], hi[0]))
    else:
        k = interleave(cells(np.where(nan[:, None], lo[None, :], X), lo, hi, BITS[dim]), BITS[dim])
    return np.where(nan, np.int64(LARGEST[dim]), k)


def order(S):
    """(keys ascending, perm, inverse): perm the stable ascending sort of the keys, inverse[perm[i]] = i."""
    k = keys(S)
    perm = np.argsort(k, kind="stable")
    inverse = np.empty_like(perm)
    inverse[perm] = np.arange(len(perm))
    return k[perm], perm, inverse


def relabel(hoods, nk, inverse, row_perm=None, own=None):
    """(out, bad) of the relabel kernel: out[i, k] = inverse[hoods[row_perm[i], k]] for k < nk[row_perm[i]] (nk None: every slot is live;
    row_perm None: the identity); the padding holds own[i] (None: i); a live entry outside 0 .. npoints - 1 is written -1 and counted."""
    hoods = np.asarray(hoods)
    n, K = hoods.shape
    npoints = len(inverse)
    rows = np.arange(n) if row_perm is None else np.asarray(row_perm)
    src = hoods[rows].astype(np.int64)
    live = np.ones((n, K), bool) if nk is None else np.arange(K)[None, :] < np.asarray(nk)[rows][:, None]
    wrong = live & ((src < 0) | (src >= npoints))
    out = np.where(wrong, -1, np.asarray(inverse)[np.where(live & ~wrong, src, 0)])
    pad = np.broadcast_to((np.arange(n) if own is None else np.asarray(own))[:, None], (n, K))
    return np.where(live, out, pad).astype(np.int32), int(wrong.sum())


def lattice(dim, p, origin, s, rng=None, npoints=None, flat=None):
    """(S, J): integer points J (n, dim) in 0 .. 2^p with both corners present (every point of the lattice when npoints is None and it is
    small, else npoints random ones), and S = origin + J * 2^s, exact for the origins and shifts of this file's tests.  flat: an axis
    on which every point has J = 0."""
    side = 2 ** p + 1
    if npoints is None:
        J = np.stack(np.meshgrid(*[np.arange(side)] * dim, indexing="ij"), axis=-1).reshape(-1, dim)
        if rng is not None:
            J = J[rng.permutation(len(J))]
    else:
        J = rng.integers(0, side, (npoints, dim))
        J[0], J[-1] = 0, side - 1
    J = J.astype(np.int64)
    if flat is not None:
        J[:, flat] = 0
    S = origin + np.ldexp(J.astype(np.float64), s)
    return S, J


def exact(S, J, origin, s):
    """True when S holds origin + J * 2^s without a rounding (the lattice's premise)."""
    from fractions import Fraction
    o, two = Fraction(float(origin)), Fraction(2) ** s
    return all(Fraction(float(v)) == o + int(j) * two for v, j in zip(np.ravel(S), np.ravel(J)))


def lattice_cases():
    """(dim, p, origin, s, flat): every origin and shift of _order_ref whose lattice is exact in float64."""
    out = []
    for dim, p in ((2, 5), (3, 3)):
        for origin, s in ((o, s) for o in ORIGINS for s in SHIFTS):
            S, J = lattice(dim, p, origin, s)
            if exact(S, J, origin, s):
                out.append((dim, p, origin, s, None))
    out += [(2, 5, 1e6, -3, 1), (3, 3, -3.0, 0, 0), (3, 3, 0.0, -400, 2)]
    return out


def lattice_cells(J, p, B):
    """The integer truth: q = J << (B - p), clamped at the upper face; 0 on a flat axis."""
    q = np.minimum(J << (B - p), 2 ** B - 1)
    flat = J.max(axis=0) == J.min(axis=0)
    q[:, flat] = 0
    return q


def permuted_dense(M, perm):
    """P M P^T: row i and column i of the result are row perm[i] and column perm[i] of M."""
    return M[np.ix_(perm, perm)]


def rehearsal(name, nb=16):
    """(as given, reordered, searched again): iterations of tests/_krylov_block_ref.solve_ref (block-nb BiCGSTAB, zero start, rtol 1e-10,
    the CPU fit's coefficients) on tests/_krylov_ref.system(name) in its random order, on P M P^T with this file's order, and on
    tests/_krylov_block_ref.morton_system(name)."""
    import _krylov_block_ref as KB
    import _krylov_ref as KR
    sy = KR.system(name)
    M = KR.dense_of(sy)
    _, perm, _ = order(sy["S"])
    counts = []
    for A, b in ((M, sy["b"]), (permuted_dense(M, perm), sy["b"][perm])):
        x, it, status, _ = KB.solve_ref(A, b, nb)
        assert status == KR.CONVERGED, (name, status)
        counts.append(it)
    ms = KB.morton_system(name)
    x, it, status, _ = KB.solve_ref(KR.dense_of(ms), ms["b"], nb)
    assert status == KR.CONVERGED, (name, status)
    return counts[0], counts[1], it
