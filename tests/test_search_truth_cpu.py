"""The exact families, the integer truth and the checkers of tests/_search_cases.py, tested without a GPU: the families are exact in
float64, the checkers accept the truth and reject each planted error, and the grid's shape (wlsqm_hip_grid_shape_host, the one
statement of what GridIndex::build lays over a cloud) keeps its budget and its ~4 points per cell on ordinary, thin, 2^+-100, 2^+-400
and one-ulp-wide boxes."""
import os

import numpy as np
import pytest

import _search_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVERY = [(name, dim) for name in SC.FAMILIES for dim in (1, 2, 3)]


@pytest.fixture(scope="module")
def whip():
    from wlsqm import _binding
    if not os.path.exists(_binding.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    import wlsqm.hip as H
    return H


@pytest.mark.parametrize("name,dim", EVERY)
def test_family_is_exact(name, dim):
    """The coordinates reproduce J, and the float d2 of a sample of pairs is the integer d2 times 2^(2s), bit for bit, in both orders of
    the sum and with the squares fused into it or not (here: separately rounded; an exact sum has one value)."""
    c = SC.case(name, dim)
    assert c.X.shape == (c.n, dim) and c.X.dtype == np.float64 and np.isfinite(c.X).all()
    assert np.array_equal(SC.integers_of(c.X, c.origin, c.s), c.J)
    if c.minus_zero is not None:
        assert np.signbit(c.X[c.minus_zero]).all() and (c.X[c.minus_zero] == 0.0).all()
    rng = np.random.default_rng(7)
    a, b = rng.integers(0, c.n, size=4000), rng.integers(0, c.n, size=4000)
    d = c.X[a] - c.X[b]
    d2 = np.zeros(len(a))
    for m in range(dim):
        d2 = d2 + d[:, m] * d[:, m]
    Jd = c.J[a] - c.J[b]
    want = np.ldexp((Jd * Jd).sum(axis=1).astype(np.float64), 2 * c.s)
    assert (Jd * Jd).sum(axis=1).max() < 2 ** 53
    assert np.array_equal(d2, want) and np.isfinite(want).all()
    assert ((want > 0) == ((Jd != 0).any(axis=1))).all()             # no squared distance of distinct points underflows


@pytest.mark.parametrize("name,dim", [("lattice", 1), ("lattice", 2), ("lattice", 3), ("duplicates", 2), ("coincident", 3), ("slab", 2)])
def test_checkers_accept_the_truth(name, dim):
    c = SC.case(name, dim)
    t = c.truth
    for k in (1, 7, c.default_k(), min(SC.KMAX, c.n - 1)):
        SC.check_knn(c.J, t.idx[:, :k], k, t)
        SC.check_knn(c.J, t.idx[:63, :k], k, t)                       # the first rows of a subset search
    for r2, max_nk in ((25, 12), (25, 100), (0.25, 5), (0, 40)):
        inside = SC.ball_counts(c.J, r2)
        nk = np.minimum(inside, max_nk)
        hoods = np.where(np.arange(max_nk)[None, :] < nk[:, None], t.idx[:, :max_nk] if t.idx.shape[1] >= max_nk else
                         np.pad(t.idx, ((0, 0), (0, max_nk - t.idx.shape[1]))), np.arange(c.n)[:, None])
        SC.check_ball(c.J, hoods, nk, r2, max_nk, t)
    SC.check_nearest(c.J, c.J, SC.nearest_truth(c.J, c.J))
    q, p = SC.ball_pairs(c.J[:200], c.J, 25)
    off = np.concatenate([[0], np.cumsum(np.bincount(q, minlength=200))])
    SC.check_lists(c.J[:200], c.J, 25, off, p[::-1][np.argsort(q[::-1], kind="stable")])      # any order inside a list


def interior(c):
    return int(np.flatnonzero((c.J == SC.LATTICE_SIDE[c.dim] // 2).all(axis=1))[0])


def test_checker_rejects_each_planted_knn_error():
    """On the 2D lattice with k = 12 an interior row is 4 + 4 + 4 points at d2 = 1, 2, 4, and the 13th distance is 5: no tie at the cut."""
    c = SC.case("lattice", 2)
    t, k, q = c.truth, 12, interior(c)
    good = t.idx[:, :k].copy()
    assert list(t.d2[q, :13]) == [1] * 4 + [2] * 4 + [4] * 4 + [5]
    SC.check_knn(c.J, good, k, t)
    swapped = good.copy(); swapped[q, [0, 1]] = swapped[q, [1, 0]]
    with pytest.raises(AssertionError, match="ascend"):
        SC.check_knn(c.J, swapped, k, t)                               # two tied entries swapped
    farther = good.copy(); farther[q, k - 1] = t.idx[q, k]
    with pytest.raises(AssertionError, match="smallest of the truth"):
        SC.check_knn(c.J, farther, k, t)                               # one neighbour replaced by the next-farther one
    repeat = good.copy(); repeat[q, 1] = repeat[q, 0]
    with pytest.raises(AssertionError, match="ascend"):
        SC.check_knn(c.J, repeat, k, t)                                # a repeated index
    own = good.copy(); own[q, 0] = q
    with pytest.raises(AssertionError, match="its own point"):
        SC.check_knn(c.J, own, k, t)                                   # the point itself
    other = good.copy(); other[q, 5] = t.idx[q, 9]
    with pytest.raises(AssertionError):
        SC.check_knn(c.J, other, k, t)                                 # a farther point in a nearer one's place
    with pytest.raises(AssertionError):
        SC.check_knn(c.J, good[:, :k - 1], k, t)                       # a missing column
    # k = 10 cuts inside the class d2 = 4: any two of its four members are legitimate, in ascending index; anything else is not
    k = 10
    cls = np.sort(t.idx[q, 8:12])
    for pair in ([0, 1], [0, 3], [2, 3], [1, 2]):
        row = t.idx[:, :k].copy(); row[q, 8:10] = cls[pair]
        SC.check_knn(c.J, row, k, t)
    row = t.idx[:, :k].copy(); row[q, 8:10] = cls[[3, 0]]
    with pytest.raises(AssertionError, match="ascend"):
        SC.check_knn(c.J, row, k, t)
    row = t.idx[:, :k].copy(); row[q, 6:8] = row[q, [7, 6]]            # inside the row a tie is not free: it is ordered by index
    with pytest.raises(AssertionError, match="ascend"):
        SC.check_knn(c.J, row, k, t)


def test_checker_rejects_each_planted_ball_error():
    """r = 5 on the 2D lattice: 80 others in the closed ball of an interior point, 12 of them ((3, 4), (5, 0), ...) on the sphere."""
    c = SC.case("lattice", 2)
    t, q, r2, max_nk = c.truth, interior(c), 25, 100
    inside = SC.ball_counts(c.J, r2)
    assert inside[q] == 80 and (t.d2[q, :80] == 25).sum() == 12 and inside.max() == 80
    nk = inside.copy()
    hoods = np.where(np.arange(max_nk)[None, :] < nk[:, None], t.idx[:, :max_nk], np.arange(c.n)[:, None])
    SC.check_ball(c.J, hoods, nk, r2, max_nk, t, inside)
    h, m = hoods.copy(), nk.copy(); h[q, 79] = q; m[q] = 79            # a sphere point dropped: what d2 < r2 would return
    with pytest.raises(AssertionError, match="nk is not"):
        SC.check_ball(c.J, h, m, r2, max_nk, t, inside)
    h = hoods.copy(); h[q, 79] = q                                     # ... dropped, the count kept
    with pytest.raises(AssertionError, match="its own point"):
        SC.check_ball(c.J, h, nk, r2, max_nk, t, inside)
    m = nk.copy(); m[q] += 1                                           # nk off by one
    with pytest.raises(AssertionError, match="nk is not"):
        SC.check_ball(c.J, hoods, m, r2, max_nk, t, inside)
    m = nk.copy(); m[0] -= 1
    with pytest.raises(AssertionError, match="nk is not"):
        SC.check_ball(c.J, hoods, m, r2, max_nk, t, inside)
    h = hoods.copy(); h[q, 90] = 0                                     # an unused slot that is not the point itself
    with pytest.raises(AssertionError, match="unused slot"):
        SC.check_ball(c.J, h, nk, r2, max_nk, t, inside)
    h = hoods.copy(); h[q, [70, 71]] = h[q, [71, 70]]                  # a whole ball is ordered by (d2, index) too
    with pytest.raises(AssertionError, match="ascend"):
        SC.check_ball(c.J, h, nk, r2, max_nk, t, inside)
    # max_nk = 12 cuts inside the class d2 = 4 ... no: 4 + 4 + 4 = 12 ends it; max_nk = 10 cuts inside it
    for max_nk in (12, 10):
        nk = np.minimum(inside, max_nk)
        hoods = np.where(np.arange(max_nk)[None, :] < nk[:, None], t.idx[:, :max_nk], np.arange(c.n)[:, None])
        SC.check_ball(c.J, hoods, nk, r2, max_nk, t, inside)
        h = hoods.copy(); h[q, max_nk - 1] = t.idx[q, 12]              # d2 = 5 in the place of a d2 = 4
        with pytest.raises(AssertionError, match="smallest of the truth"):
            SC.check_ball(c.J, h, nk, r2, max_nk, t, inside)


def test_checker_rejects_planted_nearest_and_list_errors():
    c = SC.case("lattice", 2)
    side = SC.LATTICE_SIDE[2]
    centres = 2 * SC.lattice_J(2, side - 1) + 1                        # in half steps: four cloud points tie at every centre
    J2 = 2 * c.J
    want = SC.nearest_truth(centres, J2)
    SC.check_nearest(centres, J2, want)
    d2 = SC.squared_distances(centres[:5], J2)
    assert ((d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) == 4).all()
    larger = want.copy(); larger[3] = np.flatnonzero(d2[3] == d2[3].min())[1]
    with pytest.raises(AssertionError, match="query 3"):
        SC.check_nearest(centres, J2, larger)                          # the larger index of a tie
    SC.check_nearest_far([[2 ** 60, 0]], c.J, [c.n - side])            # (46, 0) is the nearest of (2^60, 0)
    SC.check_nearest_far([[2 ** 60, 0]], c.J, [c.n - side - 1])        # (45, 46) is 1 + 2^-59 times as far: inside the roundings' bound
    with pytest.raises(AssertionError, match="far query"):
        SC.check_nearest_far([[2 ** 30, 0]], c.J, [c.n - side - 1])    # 1 + 2^-29 times as far: not
    q, p = SC.ball_pairs(c.J[:100], c.J, 25)
    off = np.concatenate([[0], np.cumsum(np.bincount(q, minlength=100))])
    SC.check_lists(c.J[:100], c.J, 25, off, p)
    sphere = np.flatnonzero(SC.squared_distances(c.J[50:51], c.J)[0][p[off[50]:off[51]]] == 25)[0] + off[50]
    off_less = off.copy(); off_less[51:] -= 1
    with pytest.raises(AssertionError, match="closed ball"):
        SC.check_lists(c.J[:100], c.J, 25, off_less, np.delete(p, sphere))     # a sphere point missing
    again = p.copy(); again[off[50]] = again[off[50] + 1]
    with pytest.raises(AssertionError, match="closed ball"):
        SC.check_lists(c.J[:100], c.J, 25, off, again)                 # a repeat


# ---- the grid's shape ----

LIVE_MIN = 2.0 ** -537            # below it the squares of an axis' differences vanish: the axis separates nothing and gets one cell
CAP = {1: 2 ** 24, 2: 16384, 3: 1024}


def boxes(dim):
    """(lo, hi, what) over ordinary, thin, scaled and one-ulp-wide boxes."""
    one = np.ones(dim)
    out = [(0.0 * one, one, "unit"), (-one, one, "centred"), (2.0 ** 20 * one, 2.0 ** 20 * one + 46 * 2.0 ** -20, "far"),
           (one, np.nextafter(one, 2.0), "one ulp wide"), (2.0 ** 20 * one, np.nextafter(2.0 ** 20 * one, np.inf), "one ulp wide, far"),
           (one, one.copy(), "a point"), (0.0 * one, 2.0 ** -1074 * one, "one denormal wide")]
    shapes = [one, np.array([1.0, 4.0, 4.0])[:dim], np.array([4.0, 1.0, 2.5])[:dim], np.array([3.3, 1.7, 1.0])[:dim]]
    for e in (0, 100, -100, 400, -400, 505, -505, 345, -341):
        for shape in shapes:
            out.append((0.0 * one, np.ldexp(shape, e), "aspect <= 4 at 2^%d" % e))
    if dim > 1:
        for thin in (1.0, 2.0 ** -20, 2.0 ** -300, 2.0 ** -600, 0.0):
            hi = 2.0 ** 20 * one; hi[-1] = thin
            out.append((0.0 * one, hi, "slab of thickness %g" % thin))
            hi = 2.0 ** 20 * one; hi[0] = thin
            out.append((0.0 * one, hi, "slab of thickness %g on axis 0" % thin))
        hi = one.copy(); hi[0] = np.nextafter(1.0, 2.0)
        out.append((one, hi, "one ulp wide on one axis, flat on the others"))
    return out


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_grid_shape_properties(whip, dim):
    worst = 0.0
    for lo, hi, what in boxes(dim):
        for n in (1, 2, 300, 1500, 4096, 4097, 10 ** 5, 10 ** 6, 2 ** 29, 2 ** 31 - 1):
            g, cell = whip.grid_shape(dim, n, lo, hi)
            tag = (what, dim, n, list(g), list(cell))
            ext = hi - lo
            live = ext >= LIVE_MIN
            cells = int(np.prod(g.astype(object)))
            assert cells <= 2 ** 27, tag
            assert (g >= 1).all() and (g <= CAP[dim]).all(), tag
            assert (cell > 0).all() and np.isfinite(1.0 / cell).all() and np.isfinite(cell).all(), tag
            assert (g[~live] == 1).all(), tag
            assert (np.abs(g[live] * cell[live] - ext[live]) <= 4 * np.spacing(ext[live])).all(), tag
            # ~4 points per cell (up to 10^6 points the target n / 4 stays clear of the axis caps and of the budget)
            if 4096 <= n <= 10 ** 6 and live.all() and ext.max() <= 4 * ext.min():
                assert (7 / 8) ** dim * n / 4 <= cells <= n / 4, tag
                worst = max(worst, 1 - cells / (n / 4))
    print("dim %d: the floors lose at most %.1f %% of the target cells (allowed %.1f %%)" % (dim, 100 * worst, 100 * (1 - (7 / 8) ** dim)))


def test_grid_shape_of_the_families_is_that_of_ordinary_clouds(whip):
    """The sizing defect: a 3D lattice at 2^-400 used to get (1024, 1024, 1024) cells (the volume underflows to 0) and at 2^345 one cell
    (it overflows).  A power of two changes nothing about a shape."""
    for dim in (1, 2, 3):
        c = SC.case("lattice", dim)
        lo, hi = c.X.min(axis=0), c.X.max(axis=0)
        g0, cell0 = whip.grid_shape(dim, c.n, lo, hi)
        assert (g0 > 1).all()
        for e in (100, -100, 345, -341, SC.extreme_exponent(dim), -SC.extreme_exponent(dim)):
            g, cell = whip.grid_shape(dim, c.n, np.ldexp(lo, e), np.ldexp(hi, e))
            assert np.array_equal(g, g0) and np.array_equal(cell, np.ldexp(cell0, e)), (dim, e, list(g), list(g0))
    for dim, want in ((2, (16384, 1)), (3, (732, 732, 1))):
        c = SC.case("slab", dim)
        g, _ = whip.grid_shape(dim, c.n, c.X.min(axis=0), c.X.max(axis=0))
        assert tuple(g) == want                                        # what the issue records of the sizing of a 1500-point slab


def test_grid_shape_rejects(whip):
    nan, inf = float("nan"), float("inf")
    for lo, hi in (([0.0, nan], [1.0, 1.0]), ([0.0, 0.0], [1.0, nan]), ([0.0, 0.0], [inf, 1.0]), ([-inf, 0.0], [1.0, 1.0]),
                   ([0.0, inf], [1.0, inf]), ([0.0, -inf], [1.0, -inf])):
        with pytest.raises(ValueError, match="non-finite coordinates"):
            whip.grid_shape(2, 100, lo, hi)
    for lo, hi in (([0.0, 0.0], [2.0 ** 520, 2.0 ** 520]), ([-1e308, 0.0], [1e308, 1.0]), ([0.0, 0.0], [2.0 ** 511.8, 2.0 ** 511.8])):
        with pytest.raises(ValueError, match="overflow"):
            whip.grid_shape(2, 100, lo, hi)
    g, cell = whip.grid_shape(2, 2209, [0.0, 0.0], [46 * 2.0 ** 505] * 2)     # `huger` in 2D is inside the domain
    assert (g > 1).all()
    with pytest.raises(ValueError):
        whip.grid_shape(2, 100, [1.0, 0.0], [0.0, 1.0])
    with pytest.raises(ValueError):
        whip.grid_shape(4, 100, [0.0] * 4, [1.0] * 4)
