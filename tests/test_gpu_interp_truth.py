"""ExpertSolver.interpolate (csrc/interp.hip, the three wlsqm_hip_expert_interpolate* entry points) and InterpolationPlan.evaluate
against the long-double truth of tests/_interp_ref.py, in 1D, 2D and 3D, for every diff 0 .. max_no + 1, with per-model orders, points
outside the cloud, points just inside a sphere and empty balls.  Two coefficient sets per dimension: the solver's own solve of a smooth
field, and a random one (held by a solver whose masks declare every DOF known, so that its solve leaves them as they are), in which no
column is small by accident and the columns beyond a model's order are not zero.

The lists are checked first (I is the brute-force nearest model; the plan's balls are cKDTree's), then the values: nearest within
64 eps T_m, continuous within eps ((64 + 4 len) sum w T + 16 sum T) / sum w (derived in tests/_interp_ref.py, measured on an fp64 replay
by tests/test_interp_ref_host.py); exactly 0 where the model lacks the diff and for diff >= max_no; NaN exactly on the empty lists.
Every test prints the largest observed ratio before it asserts."""
import numpy as np
import pytest

import _interp_ref as R

pytestmark = pytest.mark.gpu

_SOLVERS = {}


@pytest.fixture(scope="module")
def wlsqm():
    import wlsqm as W
    from wlsqm import _binding
    assert _binding.lib().wlsqm_hip_device_count() >= 1, "no HIP device: the GPU tests need a real MI355X"
    return W


def solvers(W, dim):
    """[(tag, solver, fi)]: 'solve', the fit of sin(2x) sin(2y) sin(2z) with mixed orders; 'random', every DOF known, so fi stays."""
    if dim not in _SOLVERS:
        g = R.geometry(dim)
        n, k = g["n"], g["k"]
        common = dict(dimension=dim, nk=np.full(n, k, np.int32), order=g["order"], weighting_method=np.full(n, 2, np.int32))
        a = W.ExpertSolver(knowns=np.zeros(n, np.int64), **common)
        a.prepare(xi=g["xi"], xk=g["xk"])
        fi_a = np.zeros((n, g["max_no"]))
        a.solve(fk=g["F"][g["hoods"]], fi=fi_a)
        assert np.isfinite(fi_a).all()
        b = W.ExpertSolver(knowns=((np.int64(1) << g["no"].astype(np.int64)) - 1), **common)
        b.prepare(xi=g["xi"], xk=g["xk"])
        fi_b = g["fi_random"].copy()
        b.solve(fk=g["F"][g["hoods"]], fi=fi_b)
        assert np.array_equal(fi_b, g["fi_random"])               # nothing to solve: the coefficients are the given ones
        for s in (a, b):
            s.prep_interpolate()
        _SOLVERS[dim] = [("solve", a, fi_a), ("random", b, fi_b)]
    return _SOLVERS[dim]


def _hold_nearest(what, got, g, fi, diff, I):
    T = R.truth_interpolate(g["dim"], g["S"], fi, g["order"], g["X"], diff, I=I)
    bound = R.nearest_bound(g["dim"], g["S"], fi, g["order"], g["X"], diff, I)
    gone = diff >= g["no"][I]
    assert (got[gone] == 0.0).all(), (what, diff)
    err = np.abs((got - T).astype(np.float64))
    assert (err <= bound).all(), (what, diff, int(np.argmax(err - bound)), float((err - bound).max()))
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def _hold_continuous(what, got, g, fi, diff, skip):
    """`skip`: points whose list the search may decide either way (an origin within 1e-12 r of the sphere)."""
    T = R.truth_interpolate(g["dim"], g["S"], fi, g["order"], g["X"], diff, lists=g["lists"], r=g["r"])
    bound = R.continuous_bound(g["dim"], g["S"], fi, g["order"], g["X"], diff, g["lists"], g["r"])
    assert np.array_equal(np.isnan(got)[~skip], g["empty"][~skip]), (what, diff)
    ok = ~g["empty"] & ~skip
    if diff >= g["max_no"]:
        assert (got[ok] == 0.0).all(), (what, diff)
    err = np.abs((got[ok] - T[ok]).astype(np.float64))
    assert (err <= bound[ok]).all(), (what, diff, int(np.flatnonzero(ok)[np.argmax(err - bound[ok])]), float((err - bound[ok]).max()))
    live = bound[ok] > 0
    return float((err[live] / bound[ok][live]).max()) if live.any() else 0.0


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_interpolate_nearest_against_truth(wlsqm, dim):
    """mode='nearest' with the device search and with I= given (the list-taking entry point)."""
    g = R.geometry(dim)
    for tag, s, fi in solvers(wlsqm, dim):
        worst = [0.0, 0.0]
        for diff in range(g["max_no"] + 2):
            got, I = s.interpolate(g["xq"], mode="nearest", diff=diff)
            assert np.array_equal(I, g["nearest"]), (tag, diff, np.flatnonzero(I != g["nearest"])[:8])
            worst[0] = max(worst[0], _hold_nearest("searched", got, g, fi, diff, g["nearest"]))
            got, I = s.interpolate(g["xq"], mode="nearest", diff=diff, I=g["given"])
            assert np.array_equal(I, g["given"])
            worst[1] = max(worst[1], _hold_nearest("given", got, g, fi, diff, g["given"]))
        print("dim %d %s: largest |got - truth| / (64 eps T): searched %.3f, I given %.3f" % (dim, tag, worst[0], worst[1]))


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_interpolate_continuous_against_truth(wlsqm, dim):
    """mode='continuous' with the device search: the models it averages are cKDTree's ball, or the value would not be the truth's."""
    g = R.geometry(dim)
    for tag, s, fi in solvers(wlsqm, dim):
        worst = 0.0
        for diff in range(g["max_no"] + 2):
            got, none = s.interpolate(g["xq"], mode="continuous", r=g["r"], diff=diff)
            assert got.shape == (R.NX,)
            worst = max(worst, _hold_continuous(tag, got, g, fi, diff, g["edge"]))
        print("dim %d %s: largest |got - truth| / bound = %.3f; %d empty balls, %d points on a sphere's edge"
              % (dim, tag, worst, g["empty"].sum(), g["edge"].sum()))


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_plan_against_truth(wlsqm, dim):
    """interpolation_plan(...).evaluate in both modes: its I and its lists are the truth's, then its values, all diffs in one launch; the
    random coefficients go in as fi=."""
    import torch
    g = R.geometry(dim)
    (_, s, fi_a), (_, _, fi_b) = solvers(wlsqm, dim)
    dev = torch.device("cuda", 0)
    diffs = list(range(g["max_no"] + 2))
    xq = g["xq"].copy()                                           # the shared geometry is read-only; the plan uploads a writable copy
    searched = s.interpolation_plan(xq)
    assert np.array_equal(searched.I.cpu().numpy(), g["nearest"])
    given = s.interpolation_plan(xq, I=g["given"].copy())
    ball = s.interpolation_plan(xq, mode="continuous", r=g["r"])
    off, idx = (t.cpu().numpy() for t in ball.lists())
    assert off.shape == (R.NX + 1,) and off[0] == 0 and off[-1] == len(idx)
    for m in np.flatnonzero(~g["edge"]):
        mine = idx[off[m]:off[m + 1]]
        assert len(set(mine.tolist())) == len(mine) and sorted(mine.tolist()) == sorted(g["lists"][m]), m
    for tag, fi in (("solve", fi_a), ("random", fi_b)):
        fi_d = torch.from_numpy(fi).to(dev)
        worst = [0.0, 0.0, 0.0]
        out = [p.evaluate(diffs, fi=fi_d).cpu().numpy() for p in (searched, given, ball)]
        assert all(o.shape == (len(diffs), R.NX) for o in out)
        for diff in diffs:
            worst[0] = max(worst[0], _hold_nearest("plan searched", out[0][diff], g, fi, diff, g["nearest"]))
            worst[1] = max(worst[1], _hold_nearest("plan given", out[1][diff], g, fi, diff, g["given"]))
            worst[2] = max(worst[2], _hold_continuous("plan continuous", out[2][diff], g, fi, diff, g["edge"]))
        print("dim %d %s, plan: largest |got - truth| / bound: searched %.3f, I given %.3f, continuous %.3f" % ((dim, tag) + tuple(worst)))
    for p in (searched, given, ball):
        p.close()
