"""Exact-arithmetic clouds for the neighbour searches (csrc/knn.hip, csrc/wlsqm_grid.hpp, the ball walks of csrc/interp_plan.hip), their
brute-force integer truth, and the checkers of a knn row, a ball row, a nearest index and a plan's lists.

Exactness device.  Every coordinate is origin + J * 2^s with J an int64 array, origin and s chosen so that the coordinate is exact in
float64, and |J_a - J_b| < 2^26 on every axis.  Then every difference, square and sum the kernels compute is exact, fused or not: the
kernel's d2 is the integer sum (J_a - J_b)^2 times 2^(2s), bit for bit, and the families need no tolerance.  Queries that are no cloud
points (cell centres, points outside the box) are given in the same integer units, doubled where a half step is needed.

The checkers raise AssertionError; tests/test_search_truth_cpu.py shows that they accept the truth and reject each planted error."""
import numpy as np

LATTICE_SIDE = {1: 1500, 2: 47, 3: 13}        # 1500, 2209, 2197 points: no multiple of 64, so the last wave is partial
N_RANDOM = 1500
KMAX = 213                                    # the LDS limit of knn_query_kernel
TRUTH_COLUMNS = KMAX + 1                      # the k-th and the (k + 1)-th distance of every k the library takes
CHUNK_BYTES = 64 << 20

FAMILIES = ("lattice", "lattice_far", "straddle", "negative", "random", "tiny", "huge", "tinier", "huger", "slab", "flat_axis",
            "clustered", "duplicates", "coincident")


def lattice_J(dim, side=None):
    side = LATTICE_SIDE[dim] if side is None else side
    axes = np.meshgrid(*([np.arange(side, dtype=np.int64)] * dim), indexing="ij")
    return np.stack([a.ravel() for a in axes], axis=1)


def extreme_exponent(dim):
    """`tinier` / `huger`: 2^-+400 underflows / overflows the VOLUME of a 3D box (and is harmless in 1D); in 2D that takes 2^-+505.
    The squared distances stay in range: at most 2 * 46^2 * 2^1010 < 2^1023."""
    return 505 if dim == 2 else 400


def build_family(name, dim):
    """(J, origin, s, minus_zero): the integer coordinates, the origin and the exponent of the step, and the number of the one point
    whose (zero) coordinates are written as -0.0 (or None)."""
    rng = np.random.default_rng(1000 * dim + FAMILIES.index(name))
    origin, s, minus_zero = 0.0, 0, None
    if name in ("lattice", "lattice_far", "tiny", "huge", "tinier", "huger"):
        J = lattice_J(dim)
        if name == "lattice_far":
            origin, s = 2.0 ** 20, -20
        else:
            s = {"lattice": 0, "tiny": -100, "huge": 100, "tinier": -extreme_exponent(dim), "huger": extreme_exponent(dim)}[name]
    elif name == "straddle":                   # below 2^20 the spacing of float64 is half of what it is above
        J = lattice_J(dim) - LATTICE_SIDE[dim] // 2
        origin, s = 2.0 ** 20, -20
    elif name == "negative":
        J = lattice_J(dim) - LATTICE_SIDE[dim] // 2
        minus_zero = int(np.flatnonzero((J == 0).all(axis=1))[0])
    elif name == "random":
        J = rng.integers(0, 2 ** 20, size=(N_RANDOM, dim), dtype=np.int64)
    elif name == "slab":                       # the last axis has two values: a grid of (16384, 1) or (732, 732, 1) cells
        J = rng.integers(0, 2 ** 20, size=(N_RANDOM, dim), dtype=np.int64)
        J[:, -1] = rng.integers(0, 2, size=N_RANDOM)
    elif name == "flat_axis":
        J = rng.integers(0, 2 ** 20, size=(N_RANDOM, dim), dtype=np.int64)
        J[:, 0] = 12345
    elif name == "clustered":
        J = rng.integers(0, 2 ** 20, size=(N_RANDOM, dim), dtype=np.int64)
        dense = rng.permutation(N_RANDOM)[:int(0.87 * N_RANDOM)]
        J[dense] = rng.integers(0, 2 ** 8, size=(len(dense), dim))
        J[N_RANDOM // 2] = 2 ** 24             # the outlier
    elif name == "duplicates":
        sites = np.unique(rng.integers(0, 64, size=(400, dim), dtype=np.int64), axis=0)
        sites = sites[rng.permutation(len(sites))[:60]]
        J = sites[rng.integers(0, len(sites), size=N_RANDOM)]
    elif name == "coincident":
        J = np.full((300, dim), 3, dtype=np.int64)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(J), origin, s, minus_zero


def coordinates(J, origin, s, minus_zero=None):
    """origin + J * 2^s in float64 (exact by construction; Case asserts it)."""
    X = np.ldexp(J.astype(np.float64), s) + origin
    if minus_zero is not None:
        assert (X[minus_zero] == 0.0).all()
        X[minus_zero] = -0.0
    return X


def integers_of(X, origin, s):
    """The J that `coordinates` was given, recovered from the floats (exact, or the family is not)."""
    return np.ldexp(X - origin, -s)


def squared_distances(JQ, J):
    """Integer d2[q, a] = sum_m (JQ[q, m] - J[a, m])^2 (int64)."""
    d = JQ[:, None, :] - J[None, :, :]
    return (d * d).sum(axis=2)


def chunks(nrows, ncols):
    step = max(1, CHUNK_BYTES // (8 * max(ncols, 1) * 4))     # the difference, its square, the sum and the sort's permutation
    for a in range(0, nrows, step):
        yield a, min(nrows, a + step)


class Truth:
    """Of every point of the cloud the other points in ascending (d2, index), cut to `TRUTH_COLUMNS`: idx and d2, (n, columns)."""

    def __init__(self, J):
        n = len(J)
        cols = min(n - 1, TRUTH_COLUMNS)
        self.idx = np.empty((n, cols), np.int64)
        self.d2 = np.empty((n, cols), np.int64)
        for a, b in chunks(n, n):
            d2 = squared_distances(J[a:b], J)
            d2[np.arange(b - a), np.arange(a, b)] = np.iinfo(np.int64).max     # the point itself goes last
            order = np.argsort(d2, axis=1, kind="stable")[:, :cols]             # stable: equal distances in ascending index
            self.idx[a:b] = order
            self.d2[a:b] = np.take_along_axis(d2, order, axis=1)
        self.idx.setflags(write=False)
        self.d2.setflags(write=False)


def ball_counts(J, r2, JQ=None, exclude_self=True):
    """Number of cloud points with d2 <= r2 of every query (default: every cloud point, itself excluded)."""
    Q = J if JQ is None else JQ
    out = np.empty(len(Q), np.int64)
    for a, b in chunks(len(Q), len(J)):
        out[a:b] = (squared_distances(Q[a:b], J) <= r2).sum(axis=1)
    return out - 1 if (JQ is None and exclude_self) else out


def ball_pairs(JQ, J, r2):
    """(query, point) of every pair with d2 <= r2, in ascending (query, point): the closed balls as one sorted list."""
    qs, ps = [], []
    for a, b in chunks(len(JQ), len(J)):
        q, p = np.nonzero(squared_distances(JQ[a:b], J) <= r2)
        qs.append(q + a); ps.append(p)
    return np.concatenate(qs), np.concatenate(ps)


def nearest_truth(JQ, J):
    """argmin over the cloud of (d2, index) for every query: np.argmin returns the first, the smallest index."""
    out = np.empty(len(JQ), np.int64)
    for a, b in chunks(len(JQ), len(J)):
        out[a:b] = np.argmin(squared_distances(JQ[a:b], J), axis=1)
    return out


class Case:
    """One (family, dim): J, the float cloud X (n, dim), origin, s, and — computed on first use, shared, read-only — the truth."""

    def __init__(self, name, dim):
        self.name, self.dim = name, dim
        self.J, self.origin, self.s, self.minus_zero = build_family(name, dim)
        self.n = len(self.J)
        self.X = coordinates(self.J, self.origin, self.s, self.minus_zero)
        assert np.array_equal(integers_of(self.X, self.origin, self.s), self.J), "family %s is not exact in float64" % name
        span = self.J.max(axis=0) - self.J.min(axis=0)
        assert span.max() < 2 ** 26 and self.n <= 4096 and self.n % 64 != 0
        self.J.setflags(write=False)
        self.X.setflags(write=False)
        self._truth = None

    @property
    def truth(self):
        if self._truth is None:
            self._truth = Truth(self.J)
        return self._truth

    @property
    def step(self):
        return float(np.ldexp(1.0, self.s))

    def default_k(self):
        return min(8 if self.dim == 1 else 32, self.n - 1)

    def points(self, JQ, halves=False):
        """Float coordinates of the integer queries JQ (in half steps when `halves`)."""
        return coordinates(np.asarray(JQ, dtype=np.int64), self.origin, self.s - 1 if halves else self.s)


_CASES = {}


def case(name, dim):
    if (name, dim) not in _CASES:
        _CASES[(name, dim)] = Case(name, dim)
    return _CASES[(name, dim)]


# ---- checkers ----

def check_rows(J, rows, counts, truth, queries=None, cut=None):
    """rows[i, :counts[i]] must be neighbours of query queries[i] (default i), a point of the cloud J:
      * indices in range, distinct and not the query;
      * the integer d2 of the row equal to the counts[i] smallest of the truth, entry for entry (the multiset);
      * (d2, index) strictly ascending along the row;
      * where the truth's counts[i]-th and (counts[i] + 1)-th distances differ — or `cut[i]` is False: the row is a whole ball, nothing
        was cut off — the row equals the truth row entry for entry; where they tie, any members of the tied class may fill the cut."""
    rows = np.asarray(rows, dtype=np.int64)
    counts = np.asarray(counts, dtype=np.int64)
    nq, n = len(rows), len(J)
    q = np.arange(nq) if queries is None else np.asarray(queries, dtype=np.int64)
    assert rows.ndim == 2 and counts.shape == (nq,) and q.shape == (nq,)
    assert counts.min() >= 0 and counts.max() <= min(rows.shape[1], truth.idx.shape[1]), "a count outside 0 .. the row's slots"
    used = np.arange(rows.shape[1])[None, :] < counts[:, None]
    assert ((rows >= 0) & (rows < n))[used].all(), "an index outside 0 .. n - 1"
    assert (rows != q[:, None])[used].all(), "a row holds its own point"
    safe = np.where(used, rows, 0)
    diff = J[safe] - J[q][:, None, :]
    d2 = (diff * diff).sum(axis=2)
    width = rows.shape[1]
    t_d2, t_idx = truth.d2[q][:, :width], truth.idx[q][:, :width]
    u = used[:, :t_d2.shape[1]]
    assert (d2[:, :t_d2.shape[1]] == t_d2)[u].all(), "the distances of a row are not the smallest of the truth"
    both = used[:, 1:]
    ascending = (d2[:, 1:] > d2[:, :-1]) | ((d2[:, 1:] == d2[:, :-1]) & (safe[:, 1:] > safe[:, :-1]))
    assert ascending[both].all(), "a row does not ascend strictly by (distance, index): a repeat, or ties out of order"
    # the class at the cut: unique unless the next distance of the truth equals the last one kept
    has_next = (counts > 0) & (counts < truth.d2.shape[1])
    last = truth.d2[q, np.maximum(counts, 1) - 1]
    nxt = truth.d2[q, np.minimum(counts, truth.d2.shape[1] - 1)]
    tied = has_next & (last == nxt)
    if cut is not None:
        tied &= np.asarray(cut, dtype=bool)
    exact = ~tied
    assert (safe[:, :t_idx.shape[1]] == t_idx)[u & exact[:, None]].all(), "a row with no tie at its cut differs from the truth"


def check_knn(J, hoods, k, truth, queries=None):
    hoods = np.asarray(hoods)
    assert hoods.ndim == 2 and hoods.shape[1] == k, "knn returns (queries, k)"
    check_rows(J, hoods, np.full(len(hoods), k), truth, queries)


def check_ball(J, hoods, nk, r2, max_nk, truth, inside=None):
    """hoods (n, max_nk), nk (n,) of a closed ball of integer squared radius r2 (a float holds a fractional one exactly) around every
    point.  At most max_nk others inside: nk is their number and the row is the ball in ascending (d2, index).  More: nk == max_nk
    with the knn criteria.  Unused slots hold the point itself.  `inside`: ball_counts(J, r2), when the caller has it."""
    hoods, nk = np.asarray(hoods, dtype=np.int64), np.asarray(nk, dtype=np.int64)
    n = len(J)
    assert hoods.shape == (n, max_nk) and nk.shape == (n,)
    inside = ball_counts(J, r2) if inside is None else inside
    want = np.minimum(inside, max_nk)
    assert np.array_equal(nk, want), "nk is not min(number of others in the closed ball, max_nk)"
    check_rows(J, hoods, nk, truth, cut=inside > max_nk)
    unused = np.arange(max_nk)[None, :] >= nk[:, None]
    assert (hoods == np.arange(n)[:, None])[unused].all(), "an unused slot does not hold the point's own index"


def check_nearest(JQ, J, got):
    got = np.asarray(got, dtype=np.int64)
    want = nearest_truth(np.asarray(JQ, dtype=np.int64), J)
    assert got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, "nearest: query %d got %d, the smallest (d2, index) is %d" % (bad[0], got[bad[0]], want[bad[0]])


def check_nearest_far(JQ, J, got, num=2 ** 49 + 1, den=2 ** 49):
    """Not exact: the differences of a far query are rounded.  The returned point's exact d2 must be <= (1 + 2^-49) times the minimum,
    in Python integers: the kernel's d2 carries one rounding per difference, one per square and dim - 1 in the sum, at most
    6 * 2^-53 relative in 3D, and two competing candidates double it."""
    Jo = [[int(v) for v in row] for row in np.asarray(J)]
    for q, row in enumerate(JQ):
        d2 = [sum((int(a) - b) ** 2 for a, b in zip(row, p)) for p in Jo]
        g = int(got[q])
        assert 0 <= g < len(Jo), "nearest: query %d got %d" % (q, g)
        assert d2[g] * den <= min(d2) * num, "nearest: far query %d got a point %g times as far as the nearest" % (q, d2[g] / min(d2))


def check_lists(JQ, J, r2, off, idx):
    """CSR lists of a continuous plan: list m is set-equal to the closed ball of query m, with no repeats."""
    off, idx = np.asarray(off, dtype=np.int64), np.asarray(idx, dtype=np.int64)
    nq = len(JQ)
    assert off.shape == (nq + 1,) and off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(idx), "malformed offsets"
    assert len(idx) == 0 or (idx.min() >= 0 and idx.max() < len(J)), "a list entry outside 0 .. n - 1"
    q = np.repeat(np.arange(nq), np.diff(off))
    order = np.lexsort((idx, q))
    tq, tp = ball_pairs(np.asarray(JQ, dtype=np.int64), J, r2)
    assert len(idx) == len(tq) and np.array_equal(q[order], tq) and np.array_equal(idx[order], tp), \
        "a list is not its closed ball (a member missing, a stranger, or a repeat)"
