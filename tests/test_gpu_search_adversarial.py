"""The neighbour searches on the GPU (csrc/knn.hip, csrc/wlsqm_grid.hpp, the ball walks of csrc/interp_plan.hip) against the brute-force
integer truth of tests/_search_cases.py, on clouds whose every coordinate is origin + J * 2^s: every difference, square and sum of the
kernels is exact, so every criterion here is an equality.  Lattices put ties everywhere and points on cell boundaries and on the sphere;
the other families move the cloud away from the origin, across a binade, below zero, to 2^+-100 and 2^+-400 (2D: 2^+-505, where the
box's volume under- or overflows), into a thin slab, a flat axis, a dense corner with an outlier, duplicates and one single site.

Two checks are not exact and carry a derived bound: a query 2^40 extents away (check_nearest_far: (1 + 2^-49) times the minimum) and
the weighted average of interpolate(mode='continuous') (the bound of tests/test_gpu_interp_plan.py for that operation).

r = 5 steps in 3D: the ball of an interior lattice point holds 514 others, more than the 213 a row can take, so "max_nk above the
largest ball" is min(largest ball + 1, 213) there; rows it cuts are held to the knn criteria, the others to the whole ball."""
import numpy as np
import pytest

import _search_cases as SC

EPS = float(np.finfo(np.float64).eps)
NO_POINT = 2 ** 31 - 1
EVERY = [(name, dim) for name in SC.FAMILIES for dim in (1, 2, 3)]
LATTICES = ("lattice", "lattice_far", "straddle", "negative", "tiny", "huge", "tinier", "huger")


@pytest.fixture(scope="module")
def H():
    import torch
    import wlsqm.hip as whip
    from wlsqm import _binding
    assert _binding.lib().wlsqm_hip_device_count() >= 1, "no HIP device: the GPU tests need a real MI355X"
    assert torch.cuda.is_available()
    return whip


def to_dev(X, flat=True):
    """Device tensor of the (n, dim) array X; a 1D cloud as (n,) (flat) or as (n, 1)."""
    import torch
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.shape[1] == 1 and flat:
        X = X[:, 0].copy()
    return torch.from_numpy(X.copy()).to(torch.device("cuda", 0))


_DEV = {}


def cloud(name, dim):
    """(case, its device tensor): shared by the tests, never written."""
    c = SC.case(name, dim)
    if (name, dim) not in _DEV:
        _DEV[(name, dim)] = to_dev(c.X)
    return c, _DEV[(name, dim)]


def host(t):
    return t.cpu().numpy()


# ---- knn ----

@pytest.mark.gpu
@pytest.mark.parametrize("name,dim", EVERY)
def test_knn_on_every_family(H, name, dim):
    import torch
    c, S = cloud(name, dim)
    k = c.default_k()
    hoods = H.knn(S, k)
    assert hoods.shape == (c.n, k) and hoods.dtype == torch.int32
    SC.check_knn(c.J, host(hoods), k, c.truth)
    assert torch.equal(H.knn(S, k), hoods)                          # two calls, one answer
    if dim == 1:
        assert S.dim() == 1 and torch.equal(H.knn(S.reshape(c.n, 1), k), hoods)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 7, 86, 213])
@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("name", ["lattice", "random", "duplicates"])
def test_knn_small_and_largest_k(H, name, dim, k):
    """86 is the first k whose candidate lists exceed 64 KiB of LDS (the hipFuncSetAttribute path), 213 the documented maximum."""
    import torch
    c, S = cloud(name, dim)
    hoods = H.knn(S, k)
    SC.check_knn(c.J, host(hoods), k, c.truth)
    assert torch.equal(H.knn(S, k), hoods)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("name", ["lattice", "clustered"])
def test_knn_subset_is_the_head_of_the_full_search(H, name, dim):
    import torch
    c, S = cloud(name, dim)
    k = c.default_k()
    full = H.knn(S, k)
    SC.check_knn(c.J, host(full), k, c.truth)
    for q in (1, 63, 64, 65, c.n - 1):
        part = H.knn(S, k, nquery=q)
        assert part.shape == (q, k) and torch.equal(part, full[:q]), q


@pytest.mark.gpu
def test_knn_1d_grid_beyond_2_18_cells(H):
    """The one shape too large for the families: a 1D lattice of 2^21 + 37 points gets more than 2^18 cells, where the stop rule's
    sliver grows with the cells per axis (knn.hip, head comment).  Every fourth point sits on a cell boundary.  The truth of a 1D
    lattice needs no search: the 8 nearest of an interior point i are i -+ 1 .. i -+ 4, the smaller index first."""
    import torch
    n, k = 2 ** 21 + 37, 8
    g, _ = H.grid_shape(1, n, [0.0], [float(n - 1)])
    assert g[0] > 2 ** 18
    S = torch.arange(n, dtype=torch.float64, device=torch.device("cuda", 0))
    hoods = H.knn(S, k)
    i = torch.arange(n, device=S.device)[:, None]
    steps = torch.tensor([-1, 1, -2, 2, -3, 3, -4, 4], device=S.device)[None, :]
    assert torch.equal(hoods[4:n - 4].to(torch.int64), (i + steps)[4:n - 4])
    J = np.arange(16, dtype=np.int64)[:, None]
    # the four rows at either end: their 8 nearest lie among the 16 end points, whose truth is brute force
    truth = SC.Truth(J)
    SC.check_knn(J, host(hoods[:4]), k, truth, queries=np.arange(4))
    SC.check_knn(J, host(hoods[n - 4:]).astype(np.int64) - (n - 16), k, truth, queries=np.arange(12, 16))


# ---- ball ----

@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("name", ["lattice", "lattice_far", "slab", "duplicates", "clustered"])
def test_ball(H, name, dim):
    c, S = cloud(name, dim)
    t = c.truth

    def run(r_steps, max_nk, inside):
        hoods, nk = H.ball(S, r_steps * c.step, max_nk)
        r2 = float(r_steps) ** 2
        assert (r_steps * c.step) ** 2 == r2 * c.step ** 2              # the kernel's r * r is the integer radius, scaled
        SC.check_ball(c.J, host(hoods), host(nk), r2, max_nk, t, inside)
        return host(hoods), host(nk)

    # r = 5 steps: (3, 4) and (5, 0) lie exactly on the sphere
    inside = SC.ball_counts(c.J, 25)
    above = int(min(inside.max() + 1, SC.KMAX))
    _, nk = run(5, above, inside)
    assert (nk == np.minimum(inside, above)).all()
    run(5, 12, inside)                                                  # cuts inside a tie class
    if name in ("lattice", "lattice_far"):
        on_sphere = (t.d2[:, :min(above, t.d2.shape[1])] == 25) & (np.arange(min(above, t.d2.shape[1]))[None, :] < nk[:, None])
        assert on_sphere.any(), "no row keeps a point of the sphere: the closed ball is not tested"
    # r = half a step
    inside = SC.ball_counts(c.J, 0.25)
    hoods, nk = run(0.5, 7, inside)
    if name in ("lattice", "lattice_far"):
        assert (nk == 0).all() and (hoods == np.arange(c.n)[:, None]).all()
    # r above the cloud's diameter
    inside = SC.ball_counts(c.J, 2.0 ** 54)
    assert (inside == c.n - 1).all()
    run(2.0 ** 27, 40, inside)
    if name == "duplicates":
        # r * r == 0: the ball is exactly the coincident copies
        r = 2.0 ** -600
        assert r > 0.0 and r * r == 0.0 and c.s == 0
        inside = SC.ball_counts(c.J, 0)
        assert inside.max() < SC.KMAX and inside.min() >= 1
        hoods, nk = H.ball(S, r, SC.KMAX)
        SC.check_ball(c.J, host(hoods), host(nk), 0, SC.KMAX, t, inside)


# ---- nearest ----

def exact_at_2_12_extents(c):
    """A query 2^12 extents outside the box is still exact where the box spans less than 2^14 half steps: the lattices, `duplicates` and
    `coincident`.  On `random`, `slab`, `flat_axis` and `clustered` (boxes of 2^20 .. 2^24 steps) its differences exceed 2^26 and the
    squares are rounded: there these queries go under the far-query bound (rounded_queries_at_2_12_extents).  On `huger` neither is
    possible, the squared distances of such a query overflow: test_nearest_without_an_answer has that case."""
    span = 2 * (c.J.max(axis=0) - c.J.min(axis=0))
    return int(max(span.max(), 2)) * 2 ** 12 < 2 ** 26 and c.s < 300


def rounded_queries_at_2_12_extents(c):
    """The queries 2^12 extents outside the box, along each axis, of the families where they are not exact: Python integers, in steps."""
    if exact_at_2_12_extents(c) or c.s >= 300:
        return []
    lo, hi = c.J.min(axis=0), c.J.max(axis=0)
    mid = [int(v) for v in lo + (hi - lo) // 2]
    Q = []
    for m in range(c.dim):
        span = max(int(hi[m] - lo[m]), 1)
        for far in (int(lo[m]) - 2 ** 12 * span, int(hi[m]) + 2 ** 12 * span):
            q = list(mid); q[m] = far
            Q.append(q)
    return Q


def query_sets(c):
    """Dyadic queries in HALF steps (so that cell centres are integers): {what: (nq, dim) int64}.  Every one of them is exact."""
    J2 = 2 * c.J
    lo, hi = J2.min(axis=0), J2.max(axis=0)
    span = np.maximum(hi - lo, 2)                                       # (a flat axis still moves by a step)
    mid = lo + 2 * ((hi - lo) // 4)
    out = {"own": J2}
    if c.name in LATTICES:
        out["centres"] = lo + 2 * SC.lattice_J(c.dim, SC.LATTICE_SIDE[c.dim] - 1) + 1      # 2^dim-way ties
    outside = []
    for m in range(c.dim):
        for sign in (-1, 1):
            q = mid.copy(); q[m] = (lo[m] - 2) if sign < 0 else (hi[m] + 2)                  # one step outside the box
            outside.append(q)
            if exact_at_2_12_extents(c):
                q = mid.copy(); q[m] = (lo[m] - 2 ** 12 * span[m]) if sign < 0 else (hi[m] + 2 ** 12 * span[m])
                outside.append(q)
    corner = lo - 2
    outside.append(corner)
    out["outside"] = np.array(outside, dtype=np.int64)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,dim", EVERY)
def test_nearest_exact(H, name, dim):
    """The argmin of (d2, index), exactly: on `duplicates` and `coincident` the smallest index of the site.  The queries: the cloud's
    own points, cell centres (lattices), one step outside the box, and 2^12 extents outside it — exact on the lattices, `duplicates` and
    `coincident`, under the far-query bound (1 + 2^-49, check_nearest_far) on the four families with wide boxes, absent on `huger`."""
    c, S = cloud(name, dim)
    J2 = 2 * c.J
    for what, Q in query_sets(c).items():
        X = c.points(Q, halves=True)
        assert np.array_equal(np.ldexp(X - c.origin, 1 - c.s), Q), (what, "the queries are not exact")
        got = host(H.nearest(S, to_dev(X)))
        try:
            SC.check_nearest(Q, J2, got)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (what, e))
    Q = rounded_queries_at_2_12_extents(c)
    assert bool(Q) != exact_at_2_12_extents(c) or name == "huger"
    if Q:
        X = np.array([[c.origin + float(v) * c.step for v in q] for q in Q])
        seen = [[int(round((x - c.origin) / c.step)) for x in row] for row in X]          # what the floats say
        assert seen == Q, "the coordinates of these queries are exact; only their squared distances are rounded"
        SC.check_nearest_far(Q, c.J, host(H.nearest(S, to_dev(X))))


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("name", ["lattice", "lattice_far", "negative", "tiny", "huge", "slab"])
def test_nearest_far_queries(H, name, dim):
    """2^40 extents away along each axis and along the diagonal: the cell number of such a query is far beyond int's range (cell_coord
    clamps in double), and its differences are rounded — the one bound of this search that is not an equality."""
    c, S = cloud(name, dim)
    lo, hi = c.J.min(axis=0), c.J.max(axis=0)
    span = [max(int(v), 1) for v in hi - lo]
    mid = [int(v) for v in lo + (hi - lo) // 2]
    Q = []
    for m in range(dim):
        for sign in (-1, 1):
            q = list(mid); q[m] = int(lo[m]) - 2 ** 40 * span[m] if sign < 0 else int(hi[m]) + 2 ** 40 * span[m]
            Q.append(q)
    Q.append([int(hi[m]) + 2 ** 40 * span[m] for m in range(dim)])
    Q.append([int(lo[m]) - 2 ** 40 * span[m] for m in range(dim)])
    X = np.array([[c.origin + float(v) * c.step for v in q] for q in Q])
    assert np.isfinite(X).all()
    exact = [[int(round((x - c.origin) / c.step)) for x in row] for row in X]        # what the floats say (a far J may have been rounded)
    got = host(H.nearest(S, to_dev(X)))
    SC.check_nearest_far(exact, c.J, got)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_nearest_without_an_answer(H, dim):
    """A NaN query, and a query whose squared distances overflow, get 2^31 - 1; their neighbours in the wave get their points."""
    c, S = cloud("huger", dim)
    X = c.X[:130].copy()
    X[5, 0] = np.nan
    X[64, dim - 1] = -np.nan
    X[70] = np.ldexp(1.0, 600)                                          # 2^1200 overflows
    got = host(H.nearest(S, to_dev(X)))
    bad = np.zeros(130, bool); bad[[5, 64, 70]] = True
    assert (got[bad] == NO_POINT).all()
    assert np.array_equal(got[~bad], np.arange(130)[~bad])


# ---- plans ----

@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("name", ["lattice", "lattice_far", "duplicates", "slab"])
def test_nearest_plan_is_the_nearest_search(H, name, dim):
    """plan.I equals wlsqm.hip.nearest bit for bit; with fi[:, 0] = the model's number, evaluate(0) returns the index as a float; a NaN
    query evaluates to NaN and changes nothing else."""
    import torch
    c, S = cloud(name, dim)
    sets = query_sets(c)
    Q = np.concatenate(list(sets.values()))
    X = c.points(Q, halves=True)
    Xd = to_dev(X)
    want = H.nearest(S, Xd)
    SC.check_nearest(Q, 2 * c.J, host(want))
    plan = H.InterpolationPlan(S, 0, Xd, mode="nearest")
    assert torch.equal(plan.I, want)
    fi = torch.arange(c.n, dtype=torch.float64, device=S.device).reshape(c.n, 1)
    val = plan.evaluate(0, fi=fi)
    assert torch.equal(val, want.to(torch.float64))
    Xn = X.copy(); Xn[3, 0] = np.nan; Xn[len(Xn) - 1, dim - 1] = np.nan
    plan_n = H.InterpolationPlan(S, 0, to_dev(Xn), mode="nearest")
    val_n = host(plan_n.evaluate(0, fi=fi))
    hole = np.zeros(len(Xn), bool); hole[[3, len(Xn) - 1]] = True
    assert np.isnan(val_n[hole]).all() and np.array_equal(val_n[~hole], host(val)[~hole])
    assert (host(plan_n.I)[hole] == NO_POINT).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("name", ["lattice", "lattice_far", "slab"])
def test_continuous_plan_lists_are_the_closed_balls(H, name, dim):
    """interp_plan_ball_kernel, both passes: the lists at r = 5 steps against the closed-ball truth, points of the sphere included."""
    c, S = cloud(name, dim)
    Q = np.concatenate(list(query_sets(c).values()))
    plan = H.InterpolationPlan(S, 0, to_dev(c.points(Q, halves=True)), mode="continuous", r=5 * c.step)
    off, idx = plan.lists()
    SC.check_lists(Q, 2 * c.J, 100, host(off), host(idx))             # in half steps r^2 = 100
    if name != "slab":
        on_sphere = SC.ball_counts(2 * c.J, 100, JQ=Q) - SC.ball_counts(2 * c.J, 99, JQ=Q)
        assert on_sphere.max() >= 2 * dim


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("name", ["lattice", "lattice_far"])
def test_hole_query_has_a_list_and_no_value(H, name, dim):
    """A lattice site removed from the cloud, asked with r = 1 step: the list is exactly the 2 dim face neighbours, all ON the sphere, so
    every weight is 0 and the value is 0 / 0 = NaN with a non-empty list."""
    import torch
    c, _ = cloud(name, dim)
    gone = int(np.flatnonzero((c.J == c.J.min(axis=0) + SC.LATTICE_SIDE[dim] // 2).all(axis=1))[0])
    keep = np.arange(c.n) != gone
    J = c.J[keep]
    S = to_dev(c.X[keep])
    Q = np.concatenate([c.J[gone:gone + 1], J[:70]])
    plan = H.InterpolationPlan(S, 0, to_dev(c.points(Q)), mode="continuous", r=c.step)
    off, idx = host(plan.lists()[0]), host(plan.lists()[1])
    SC.check_lists(Q, J, 1, off, idx)
    mine = idx[off[0]:off[1]]
    assert len(mine) == 2 * dim and (((J[mine] - c.J[gone]) ** 2).sum(axis=1) == 1).all()
    val = host(plan.evaluate(0, fi=torch.ones((len(J), 1), dtype=torch.float64, device=S.device)))
    assert np.isnan(val[0]) and (val[1:] == 1.0).all()                 # a cloud point has itself at weight 1 and its neighbours at 0


# ---- ExpertSolver.interpolate(mode='continuous'): interp_ball_kernel, the third copy of the walk ----

@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("name", ["lattice", "slab"])
def test_interpolate_continuous_against_the_truth_lists(H, name, dim):
    """Order-0 models (the value of a model is its fi[0] everywhere) fitted on the truth's 4 nearest neighbours; fi is read back after the
    solve, and the weighted average is computed in numpy over the truth's closed balls, with the weights (1 - sqrt(d2 / r2))^2 of exact
    integer d2.  Bound (tests/test_gpu_interp_plan.py, continuous): (128 + 4 len) eps sum(w |fi0|) / sum(w).  NaN exactly where
    sum(w) == 0: no model in range, or every model in range on the sphere."""
    import wlsqm
    c, _ = cloud(name, dim)
    n, t = c.n, c.truth
    hoods = t.idx[:, :4]
    F = 1.0 + np.sin(np.arange(n) * 0.37)
    xi = c.X[:, 0].copy() if dim == 1 else c.X
    xk = c.X[hoods][:, :, 0].copy() if dim == 1 else c.X[hoods]
    s = wlsqm.ExpertSolver(dimension=dim, nk=np.full(n, 4, np.int32), order=np.zeros(n, np.int32), knowns=np.zeros(n, np.int64),
                           weighting_method=np.full(n, wlsqm.WEIGHT_UNIFORM, np.int32))
    s.prepare(xi=xi, xk=xk)
    fi = np.zeros((n, 1))
    s.solve(fk=F[hoods], fi=fi)
    s.prep_interpolate()
    lo, hi = c.J.min(axis=0), c.J.max(axis=0)
    mid = lo + (hi - lo) // 2
    extra = []
    for m in range(dim):
        q = mid.copy(); q[m] = lo[m] - 5; extra.append(q)               # on a lattice: one model in range, on the sphere
        q = mid.copy(); q[m] = hi[m] + 5; extra.append(q)
        q = mid.copy(); q[m] = hi[m] + 6; extra.append(q)               # none in range
    Q = np.concatenate([c.J, np.array(extra, dtype=np.int64)])
    X = c.points(Q)
    got, _ = s.interpolate(X[:, 0].copy() if dim == 1 else X, mode="continuous", r=5 * c.step, diff=0)
    qs, ps = SC.ball_pairs(Q, c.J, 25)
    d2 = ((Q[qs] - c.J[ps]) ** 2).sum(axis=1)
    w = (1.0 - np.sqrt(d2 / 25.0)) ** 2
    f0 = fi[ps, 0]
    length = np.bincount(qs, minlength=len(Q))
    sum_w = np.bincount(qs, weights=w, minlength=len(Q))
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = np.bincount(qs, weights=w * f0, minlength=len(Q)) / sum_w
        bound = (128 + 4 * length) * EPS * np.bincount(qs, weights=w * np.abs(f0), minlength=len(Q)) / sum_w
    assert np.isfinite(fi).all(), "an order-0 model with uniform weights is the mean of its data"
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(np.isnan(got), sum_w == 0)
    assert (sum_w[:n] > 0).all() and (sum_w[n:] == 0).any()
    if name == "lattice":
        assert ((sum_w == 0) & (length > 0)).any(), "no query has all its models on the sphere"
    ok = ~np.isnan(ref)
    err = np.abs(got[ok] - ref[ok])
    print("%s %dD: %d queries, %d NaN, largest |got - ref| / bound = %.3f" % (name, dim, len(Q), int((~ok).sum()),
          float((err[bound[ok] > 0] / bound[ok][bound[ok] > 0]).max()) if (bound[ok] > 0).any() else 0.0))
    assert (err <= bound[ok]).all(), float((err - bound[ok]).max())


# ---- error paths ----

def small(H):
    c, S = cloud("lattice", 2)
    return c, S


def still_works(H):
    c, S = small(H)
    SC.check_knn(c.J, host(H.knn(S, 5)), 5, c.truth)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["k = 0", "k = n", "k = 214", "nquery = 0", "nquery = n + 1", "radius 0", "radius -1", "radius NaN"])
def test_argument_errors(H, what):
    c, S = small(H)
    n = c.n
    with pytest.raises(ValueError, match={"k": "k must be in|k too large", "n": "nquery must be", "r": "radius must be"}[what[0]]):
        if what == "k = 0":
            H.knn(S, 0)
        elif what == "k = n":
            H.knn(S, n)
        elif what == "k = 214":
            H.knn(S, 214)
        elif what == "nquery = 0":
            H.knn(S, 5, nquery=0)
        elif what == "nquery = n + 1":
            H.knn(S, 5, nquery=n + 1)
        else:
            H.ball(S, {"radius 0": 0.0, "radius -1": -1.0, "radius NaN": float("nan")}[what], 10)
    still_works(H)


NONFINITE = [("nan", 0), ("nan", "middle"), ("nan", -1), ("-nan", 0), ("-nan", "middle"), ("-nan", -1), ("inf", "middle"), ("-inf", "middle"),
             ("inf", "axis")]


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("value,where", NONFINITE)
def test_non_finite_coordinates_are_rejected(H, value, where, dim):
    """A NaN of either sign at the first, a middle or the last point, an infinity in one point, and +inf in EVERY point on one axis (lo ==
    hi == inf, whose difference is a NaN that compares false): each is 'non-finite coordinates' from all four searches."""
    c, S = cloud("lattice", dim)
    X = c.X.copy()
    v = {"nan": np.nan, "-nan": -np.nan, "inf": np.inf, "-inf": -np.inf}[value]
    assert value not in ("nan", "-nan") or np.signbit(v) == (value == "-nan")
    if where == "axis":
        X[:, dim - 1] = v
    else:
        X[c.n // 2 + 1 if where == "middle" else where, dim - 1] = v
    B = to_dev(X)
    with pytest.raises(ValueError, match="non-finite coordinates"):
        H.knn(B, 3)
    with pytest.raises(ValueError, match="non-finite coordinates"):
        H.ball(B, 1.0, 5)
    with pytest.raises(ValueError, match="non-finite coordinates"):
        H.nearest(B, S[:10].clone())
    with pytest.raises(ValueError, match="non-finite coordinates"):
        H.InterpolationPlan(B, 0, S[:10].clone(), mode="continuous", r=1.0)
    still_works(H)


@pytest.mark.gpu
def test_overflowing_squared_distances_are_rejected(H):
    """A 2D cloud scaled by 2^520: every coordinate is finite and every squared distance inf.  It used to return rows filled with the
    point's own index."""
    c, _ = cloud("lattice", 2)
    B = to_dev(np.ldexp(c.X, 520))
    assert np.isfinite(host(B)).all()
    with pytest.raises(ValueError, match="overflow"):
        H.knn(B, 3)
    with pytest.raises(ValueError, match="overflow"):
        H.ball(B, 2.0 ** 521, 5)
    with pytest.raises(ValueError, match="overflow"):
        H.nearest(B, B[:10].clone())
    still_works(H)
