"""Interpolation plans on the GPU (csrc/interp_plan.hip; wlsqm.hip.InterpolationPlan, ExpertSolver.interpolation_plan): the plan's
search and its multi-diff evaluation against the existing per-call route (ExpertSolver.interpolate and the list-taking C entry point),
and the rule that a value does not depend on what else a call asks for.

Bounds.  Nearest: |got - ref| <= 128 eps T_m with T_m = sum_a |fi[I_m, a]| |monomial_a(x_m - xi[I_m]) / factorials| over the terms
that survive the diff — at most 35 terms of at most 3 roundings each, in two implementations.  Continuous: the same per model, plus
the weighted sum over the len_m models of the list: (128 + 4 len_m) eps (sum_w w T) / sum_w w.  Both are derived, not measured; every
test prints the largest observed ratio before it asserts."""
import gc

import numpy as np
import pytest

EPS = float(np.finfo(np.float64).eps)
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
NX = 3000 + 37                     # 47 full waves and a partial one
RADIUS = {1: 0.004, 2: 0.03, 3: 0.08}


@pytest.fixture(scope="module")
def wlsqm():
    import wlsqm as W
    from wlsqm import _binding
    assert _binding.lib().wlsqm_hip_device_count() >= 1, "no HIP device: the GPU tests need a real MI355X"
    return W


def scaled_monomials(dim, dx):
    """c[:, b] = prod_m dx[:, m]^e / e! for the exponents of DOF b."""
    c = np.ones((dx.shape[0], len(EXPONENTS[dim])))
    for b, e in enumerate(EXPONENTS[dim]):
        for m in range(dim):
            c[:, b] *= dx[:, m] ** e[m] / FACT[e[m]]
    return c


def term_sum(dim, rows, no, dx, diff):
    """T = sum over the terms a < no that survive `diff` of |rows[:, a]| |c[:, index(P_a - P_diff)]|."""
    E = EXPONENTS[dim]
    index = {e: b for b, e in enumerate(E)}
    c = np.abs(scaled_monomials(dim, dx))
    T = np.zeros(dx.shape[0])
    if diff >= len(E):
        return T
    for a in range(min(rows.shape[1], len(E))):
        e = tuple(E[a][m] - E[diff][m] for m in range(3))
        if min(e) < 0:
            continue
        T += np.where(a < no, np.abs(rows[:, a]) * c[:, index[e]], 0.0)
    return T


_GEOMETRY = {}


def geometry(wlsqm, dim):
    """One solved ExpertSolver per dimension, per-model orders mixed over 0..4 (3D: 0..3, 30 neighbours do not carry the 35 unknowns of
    order 4), and NX query points of which some lie outside the cloud's bounding box.  Shared by the tests; nothing modifies it."""
    if dim in _GEOMETRY:
        return _GEOMETRY[dim]
    import scipy.spatial
    import torch
    n, k, top = 4000, {1: 8, 2: 24, 3: 30}[dim], {1: 4, 2: 4, 3: 3}[dim]
    rng = np.random.default_rng(5 + dim)
    S = rng.uniform(0.0, 1.0, size=(n, dim))
    F = np.sin(2.0 * S).prod(axis=1)
    _, hoods = scipy.spatial.cKDTree(S).query(S, k + 1)
    hoods = hoods[:, 1:]
    order = rng.integers(0, top + 1, size=n).astype(np.int32)
    max_no = NDOF[dim][top]
    xi = S[:, 0].copy() if dim == 1 else S
    xk = S[hoods][:, :, 0].copy() if dim == 1 else S[hoods]
    s = wlsqm.ExpertSolver(dimension=dim, nk=np.full(n, k, np.int32), order=order, knowns=np.zeros(n, np.int64),
                           weighting_method=np.full(n, 2, np.int32))
    s.prepare(xi=xi, xk=xk)
    fi = np.zeros((n, max_no))
    s.solve(fk=F[hoods], fi=fi)
    s.prep_interpolate()
    assert np.isfinite(fi).all()
    X = rng.uniform(-0.2, 1.2, size=(NX, dim))
    xq = X[:, 0].copy() if dim == 1 else X
    dev = torch.device("cuda", 0)
    g = dict(n=n, k=k, S=S, F=F, hoods=hoods, order=order, no=np.array(NDOF[dim])[order], max_no=max_no, solver=s, fi=fi, X=X, xq=xq,
             xq_d=torch.from_numpy(xq).to(dev), fi_d=torch.from_numpy(fi).to(dev), dev=dev, xi=xi, xk=xk)
    _GEOMETRY[dim] = g
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_nearest_plan_against_interpolate(wlsqm, dim):
    """The plan finds the same model per point as interpolate(mode='nearest') and evaluates every diff within 128 eps T_m of it;
    exactly 0 where the chosen model does not have the diff."""
    g = geometry(wlsqm, dim)
    s = g["solver"]
    plan = s.interpolation_plan(g["xq_d"])
    assert plan.nx == NX and plan.mode == "nearest" and plan.r is None and plan.memory_used() > 0
    I = plan.I.cpu().numpy()
    rows, no, dx = g["fi"][I], g["no"][I], g["X"] - g["S"][I]
    assert (dx.min(axis=1) < -0.05).any() or (dx.max(axis=1) > 0.05).any()        # some points lie outside the cloud
    worst = 0.0
    for diff in range(g["max_no"]):
        ref, I_ref = s.interpolate(g["xq"], mode="nearest", diff=diff)
        assert np.array_equal(I, I_ref)
        got = plan.evaluate(diff).cpu().numpy()
        assert got.shape == (NX,)
        T = term_sum(dim, rows, no, dx, diff)
        err = np.abs(got - ref)
        worst = max(worst, float((err[T > 0] / (EPS * T[T > 0])).max()) if (T > 0).any() else 0.0)
        assert (err <= 128 * EPS * T).all(), (diff, float((err - 128 * EPS * T).max()))
        gone = diff >= no
        assert gone.any() or diff == 0
        assert (got[gone] == 0.0).all() and (ref[gone] == 0.0).all()
    print("dim %d nearest: largest |got - ref| / (eps T) = %.2f (bound 128)" % (dim, worst))
    # a numpy x is uploaded once and gives the same plan
    plan_np = s.interpolation_plan(g["xq"])
    assert np.array_equal(plan_np.I.cpu().numpy(), I)
    assert np.array_equal(plan_np.evaluate(1).cpu().numpy(), plan.evaluate(1).cpu().numpy(), equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["nearest", "continuous"])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_a_value_does_not_depend_on_its_companions(wlsqm, dim, mode):
    """Bit for bit: a diff alone, among all of them, in a shuffled list with a repeat; a field alone or in a stack; fi=None against
    the solve's coefficients passed explicitly."""
    import torch
    g = geometry(wlsqm, dim)
    s, max_no = g["solver"], g["max_no"]
    plan = s.interpolation_plan(g["xq_d"], mode=mode, r=RADIUS[dim] if mode == "continuous" else None)
    every = plan.evaluate(list(range(max_no)))
    assert every.shape == (max_no, NX)
    rng = np.random.default_rng(17)
    shuffled = [int(d) for d in rng.permutation(max_no)] + [0, max_no - 1, max_no + 3, -2]
    mixed = plan.evaluate(shuffled)
    for d in range(max_no):
        alone = plan.evaluate([d])
        assert alone.shape == (1, NX)
        assert torch.equal(alone[0].view(torch.int64), every[d].view(torch.int64)), d
        assert torch.equal(plan.evaluate(d).view(torch.int64), every[d].view(torch.int64)), d
    for j, d in enumerate(shuffled):
        if 0 <= d < max_no:
            assert torch.equal(mixed[j].view(torch.int64), every[d].view(torch.int64)), (j, d)
    # a diff nobody has: 0 where the point has a model, NaN where it has none (as interpolate())
    nobody = mixed[len(shuffled) - 2:]
    assert torch.equal(torch.isnan(nobody[0]), torch.isnan(every[0])) and torch.equal(torch.isnan(nobody[1]), torch.isnan(every[0]))
    assert float(torch.nan_to_num(nobody, nan=0.0).abs().max()) == 0.0
    # fi=None is the latest solve; the same coefficients passed explicitly
    explicit = plan.evaluate(list(range(max_no)), fi=g["fi_d"])
    assert torch.equal(explicit.view(torch.int64), every.view(torch.int64))
    # a field alone or in a stack (the second field a non-contiguous view of a wider array)
    wide = torch.from_numpy(rng.standard_normal((g["n"], max_no + 3))).to(g["dev"])
    stack = torch.stack([g["fi_d"], wide[:, :max_no].contiguous(), -g["fi_d"]])
    diffs = [0, max_no - 1, 1]
    out = plan.evaluate(diffs, fi=stack)
    assert out.shape == (3, 3, NX)
    for f in range(3):
        assert torch.equal(out[f].view(torch.int64), plan.evaluate(diffs, fi=stack[f]).view(torch.int64)), f
        assert torch.equal(plan.evaluate(1, fi=stack)[f].view(torch.int64), plan.evaluate(1, fi=stack[f]).view(torch.int64)), f
    assert torch.equal(out[1].view(torch.int64), plan.evaluate(diffs, fi=wide[:, :max_no]).view(torch.int64))
    assert torch.equal(out[0].view(torch.int64), every[diffs].view(torch.int64))
    # a preallocated out with room to spare between the rows
    buf = torch.full((3, 5, NX + 11), 7.0, dtype=torch.float64, device=g["dev"])
    ret = plan.evaluate(diffs, fi=stack, out=buf[:, 1:4, :NX])
    assert ret.data_ptr() == buf[:, 1:4, :NX].data_ptr()
    assert torch.equal(buf[:, 1:4, :NX].view(torch.int64), out.view(torch.int64))
    assert float(buf[:, 0].min()) == 7.0 and float(buf[:, 4].min()) == 7.0 and float(buf[:, :, NX:].min()) == 7.0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["nearest", "continuous"])
def test_all_35_diffs_of_3d_order_4_equal_35_single_calls(wlsqm, mode):
    """The largest ndiff: a standalone plan over 3D order-4 models, all 35 derivatives in one launch against 35 launches of one."""
    import torch
    import wlsqm.hip as whip
    g = geometry(wlsqm, 3)
    rng = np.random.default_rng(35)
    xi_d = torch.from_numpy(g["S"]).to(g["dev"])
    fi_d = torch.from_numpy(rng.standard_normal((g["n"], 35))).to(g["dev"])
    plan = whip.InterpolationPlan(xi_d, 4, g["xq_d"], mode=mode, r=RADIUS[3] if mode == "continuous" else None)
    every = plan.evaluate(list(range(35)), fi=fi_d)
    assert every.shape == (35, NX)
    holes = torch.isnan(every[0])
    assert bool(holes.any()) == (mode == "continuous")
    for d in range(35):
        assert torch.equal(plan.evaluate(d, fi=fi_d).view(torch.int64), every[d].view(torch.int64)), d
        assert torch.equal(torch.isnan(every[d]), holes)
        assert float(every[d][~holes].abs().max()) > 0.0
    with pytest.raises(ValueError, match="at most 35"):
        plan.evaluate(list(range(36)), fi=fi_d)
    with pytest.raises(RuntimeError):
        plan.evaluate(0)                                           # no solver behind a standalone plan
    with pytest.raises(ValueError):
        plan.evaluate(0, fi=fi_d[:, :20])                          # order 4 needs 35 columns
    assert plan.evaluate([], fi=fi_d).shape == (0, NX)               # ndiff == 0: nothing happens


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_continuous_plan_lists_and_values(wlsqm, dim):
    """The lists are cKDTree's balls (set-equal per point), NaN sits exactly on the empty lists, and the values agree with
    interpolate(mode='continuous') (another summation order) and, per point, with the list-taking entry point fed with the plan's
    own lists."""
    import scipy.spatial
    import torch
    import wlsqm._binding as B
    g = geometry(wlsqm, dim)
    s, X, S, r, max_no = g["solver"], g["X"], g["S"], RADIUS[dim], g["max_no"]
    plan = s.interpolation_plan(g["xq_d"], mode="continuous", r=r)
    assert plan.mode == "continuous" and plan.r == r and plan.I is None
    off_d, idx_d = plan.lists()
    off, idx = off_d.cpu().numpy(), idx_d.cpu().numpy()
    assert off.shape == (NX + 1,) and off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(idx)
    tree = scipy.spatial.cKDTree(S)
    lists = scipy.spatial.cKDTree(X).query_ball_tree(tree, r=r)
    # points with an origin within 1e-12 r of the sphere may fall either way: at most 0.1 % of the points
    edge = tree.query_ball_point(X, r * (1 + 1e-12), return_length=True) != tree.query_ball_point(X, r * (1 - 1e-12), return_length=True)
    print("dim %d continuous: %d of %d points have an origin within 1e-12 r of the sphere" % (dim, int(edge.sum()), NX))
    assert edge.sum() <= 0.001 * NX
    for m in range(NX):
        if not edge[m]:
            mine = idx[off[m]:off[m + 1]]
            assert len(set(mine)) == len(mine) and sorted(mine) == sorted(lists[m]), m
    length = np.diff(off)
    empty = length == 0
    assert empty.any() and (~empty).sum() > 1000
    # a second plan of the same inputs holds the same lists, entry for entry
    off2, idx2 = s.interpolation_plan(g["xq_d"].clone(), mode="continuous", r=r).lists()
    assert torch.equal(off2, off_d) and torch.equal(idx2, idx_d)
    # per list entry: weight and term sum, for the per-point bound
    pt = np.repeat(np.arange(NX), length)
    dx = X[pt] - S[idx]
    w = (1.0 - np.sqrt((dx * dx).sum(axis=1) / (r * r))) ** 2
    sum_w = np.bincount(pt, weights=w, minlength=NX)
    xv = np.ascontiguousarray(X)
    worst = 0.0
    for diff in (0, 1, max_no - 1):
        got = plan.evaluate(diff).cpu().numpy()
        assert np.array_equal(np.isnan(got), empty)
        ref, _ = s.interpolate(g["xq"], mode="continuous", r=r, diff=diff)
        same = ~empty & ~edge
        assert np.array_equal(np.isnan(ref[~edge]), empty[~edge])
        scale = np.abs(ref[same]).max()
        assert np.abs(got[same] - ref[same]).max() <= 1e-12 * max(scale, 1.0)
        per = np.empty(NX)
        B.check(B.lib().wlsqm_hip_expert_interpolate(s._handle, xv.ctypes.data, dim, NX, None, off.ctypes.data, idx.ctypes.data,
                                                     float(r), int(diff), per.ctypes.data))
        assert np.array_equal(np.isnan(per), empty)
        T = term_sum(dim, g["fi"][idx], g["no"][idx], dx, diff)
        bound = (128 + 4 * length[~empty]) * EPS * np.bincount(pt, weights=w * T, minlength=NX)[~empty] / sum_w[~empty]
        err = np.abs(got[~empty] - per[~empty])
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        assert (err <= bound).all(), (diff, float((err - bound).max()))
    print("dim %d continuous: largest |got - per-point reference| / bound = %.3f" % (dim, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_given_models_and_strided_points(wlsqm, dim):
    """I with -1 and nmodels entries gives NaN exactly there and the searched plan's values elsewhere; a column slice of a wider
    tensor as x equals its contiguous copy."""
    import torch
    g = geometry(wlsqm, dim)
    s, n, diffs = g["solver"], g["n"], [0, 1, g["max_no"] - 1]
    plan = s.interpolation_plan(g["xq_d"])
    want = plan.evaluate(diffs)
    I = plan.I.clone()
    given = s.interpolation_plan(g["xq_d"], I=I).evaluate(diffs)
    assert torch.equal(given.view(torch.int64), want.view(torch.int64))
    bad = torch.zeros(NX, dtype=torch.bool, device=g["dev"])
    bad[3::97] = True
    I_bad = I.clone()
    I_bad[3::194] = -1
    I_bad[100::194] = n
    plan_bad = s.interpolation_plan(g["xq_d"], I=I_bad)
    assert torch.equal(plan_bad.I, I_bad)
    got = plan_bad.evaluate(diffs)
    assert torch.equal(torch.isnan(got), bad.expand(3, NX))
    assert torch.equal(got[:, ~bad].view(torch.int64), want[:, ~bad].view(torch.int64))
    got_np = s.interpolation_plan(g["xq"], I=I_bad.cpu().numpy()).evaluate(diffs)          # numpy x and I are uploaded once
    assert torch.equal(torch.nan_to_num(got_np, nan=-1.0), torch.nan_to_num(got, nan=-1.0))
    with pytest.raises(ValueError):
        s.interpolation_plan(g["xq_d"], I=I[:-1])
    with pytest.raises(ValueError):
        s.interpolation_plan(g["xq_d"], mode="continuous", r=RADIUS[dim], I=I)
    # strided x
    wide = torch.full((NX, dim + 3), 9.0, dtype=torch.float64, device=g["dev"])
    if dim == 1:
        wide[:, 2] = g["xq_d"]
        x_view = wide[:, 2]
    else:
        wide[:, 2:2 + dim] = g["xq_d"]
        x_view = wide[:, 2:2 + dim]
    assert not x_view.is_contiguous()
    for mode, r in (("nearest", None), ("continuous", RADIUS[dim])):
        a = s.interpolation_plan(x_view, mode=mode, r=r)
        b = s.interpolation_plan(x_view.contiguous(), mode=mode, r=r)
        ea, eb = a.evaluate(diffs), b.evaluate(diffs)
        assert torch.equal(torch.isnan(ea), torch.isnan(eb))
        assert torch.equal(torch.nan_to_num(ea, nan=0.0).view(torch.int64), torch.nan_to_num(eb, nan=0.0).view(torch.int64))
        if mode == "nearest":
            assert torch.equal(a.I, plan.I)


@pytest.mark.gpu
def test_standalone_plan_over_fit_many_device(wlsqm):
    """No solver object: InterpolationPlan(xi, order, x) over the coefficients of wlsqm.hip.fit_many_device equals the solver-bound
    plan of the same geometry bit for bit, with a per-model order tensor."""
    import torch
    import wlsqm.hip as whip
    g = geometry(wlsqm, 2)
    dev, n, k, max_no = g["dev"], g["n"], g["k"], g["max_no"]
    xi_d = torch.from_numpy(g["S"]).to(dev)
    xk_d = torch.from_numpy(g["xk"]).to(dev)
    fk_d = torch.from_numpy(g["F"][g["hoods"]]).to(dev)
    order_d = torch.from_numpy(g["order"]).to(dev)
    fi_d = torch.zeros((n, max_no), dtype=torch.float64, device=dev)
    whip.fit_many_device(2, order_d, xk_d, fk_d, torch.full((n,), k, dtype=torch.int32, device=dev), xi_d, fi_d,
                         torch.zeros(n, dtype=torch.int64, device=dev), torch.full((n,), 2, dtype=torch.int32, device=dev))
    diffs = list(range(max_no))
    for mode, r in (("nearest", None), ("continuous", RADIUS[2])):
        alone = whip.InterpolationPlan(xi_d, order_d, g["xq_d"], mode=mode, r=r)
        bound = g["solver"].interpolation_plan(g["xq_d"], mode=mode, r=r)
        a, b = alone.evaluate(diffs, fi=fi_d), bound.evaluate(diffs, fi=fi_d)
        assert torch.equal(torch.isnan(a), torch.isnan(b))
        assert torch.equal(torch.nan_to_num(a, nan=0.0).view(torch.int64), torch.nan_to_num(b, nan=0.0).view(torch.int64))
        if mode == "nearest":
            assert torch.equal(alone.I, bound.I)
        else:
            assert all(torch.equal(p, q) for p, q in zip(alone.lists(), bound.lists()))
        assert alone.memory_used() == bound.memory_used()
    # and these coefficients are a fit of the field: the patched model follows sin(2x) sin(2y) inside the cloud
    inside = (g["X"].min(axis=1) > 0.05) & (g["X"].max(axis=1) < 0.95)
    val = bound.evaluate(0, fi=fi_d).cpu().numpy()
    ok = inside & ~np.isnan(val)
    assert ok.sum() > 500 and np.abs(val[ok] - np.sin(2.0 * g["X"][ok]).prod(axis=1)).max() < 0.2
    with pytest.raises(ValueError):
        whip.InterpolationPlan(xi_d, 7, g["xq_d"])
    with pytest.raises(ValueError):
        whip.InterpolationPlan(xi_d, torch.full((n,), 5, dtype=torch.int32, device=dev), g["xq_d"])


@pytest.mark.gpu
def test_solve_and_evaluate_replay_from_one_graph(wlsqm):
    """fi[:, 0] = u; solve_device; evaluate([0, 1, 2]) captured as one linear graph and replayed with two different fields: the buffer
    holds what the eager sequence gives each time — the evaluation neither allocates nor synchronises."""
    import scipy.spatial
    import torch
    n, k, order = 2000, 16, 2
    rng = np.random.default_rng(11)
    S = rng.uniform(0.0, 1.0, size=(n, 2))
    _, hoods = scipy.spatial.cKDTree(S).query(S, k + 1)
    hoods = hoods[:, 1:]
    dev = torch.device("cuda", 0)
    s = wlsqm.ExpertSolver(dimension=2, nk=np.full(n, k, np.int32), order=np.full(n, order, np.int32),
                           knowns=np.full(n, wlsqm.b2_F, np.int64), weighting_method=np.full(n, wlsqm.WEIGHT_CENTER, np.int32))
    s.prepare(xi=S, xk=S[hoods])
    X_d = torch.from_numpy(rng.uniform(0.0, 1.0, size=(64 * 9 + 37, 2))).to(dev)
    nx = X_d.shape[0]
    plan = s.interpolation_plan(X_d)
    with pytest.raises(RuntimeError):
        plan.evaluate(0)                                           # nothing solved yet
    S_d, h_d = torch.from_numpy(S).to(dev), torch.from_numpy(hoods).to(dev)
    u = torch.empty(n, dtype=torch.float64, device=dev)
    fk = torch.empty((n, k), dtype=torch.float64, device=dev)
    fi = torch.zeros((n, 6), dtype=torch.float64, device=dev)
    buf = torch.zeros((3, nx), dtype=torch.float64, device=dev)

    def step():
        fi[:, 0] = u
        s.solve_device(fk, fi)
        plan.evaluate([0, 1, 2], out=buf)

    def field(t):
        return torch.sin(np.pi * (S_d[:, 0] - t)) * torch.cos(np.pi * S_d[:, 1])

    u.copy_(field(0.0)); fk.copy_(u[h_d])
    step()                                                           # warm-up outside the capture
    torch.cuda.synchronize()
    buf.fill_(-7.0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        step()
    torch.cuda.synchronize()
    assert float(buf.min()) == -7.0 and float(buf.max()) == -7.0      # captured, not run
    for t in (0.3, 0.7):
        u.copy_(field(t)); fk.copy_(u[h_d])
        graph.replay()
        torch.cuda.synchronize()
        got = buf.clone()
        buf.fill_(-7.0)
        step()
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int64), buf.view(torch.int64))
        Xc = X_d.cpu().numpy()
        inside = torch.from_numpy((np.abs(Xc - 0.5) < 0.4).all(axis=1)).to(dev)
        exact = torch.sin(np.pi * (X_d[:, 0] - t)) * torch.cos(np.pi * X_d[:, 1])
        assert float((got[0] - exact)[inside].abs().max()) < 1e-2    # the field of THIS replay (truncation error only)


@pytest.mark.gpu
def test_plan_outlives_its_solver(wlsqm):
    """The plan holds its own copies: valid with an explicit fi after the solver is closed and deleted; close() twice is harmless;
    evaluate() after close raises."""
    import scipy.spatial
    import torch
    n, k = 600, 12
    rng = np.random.default_rng(3)
    S = rng.uniform(0.0, 1.0, size=(n, 2))
    _, hoods = scipy.spatial.cKDTree(S).query(S, k + 1)
    hoods = hoods[:, 1:]
    s = wlsqm.ExpertSolver(dimension=2, nk=np.full(n, k, np.int32), order=np.full(n, 2, np.int32), knowns=np.zeros(n, np.int64),
                           weighting_method=np.full(n, 2, np.int32))
    with pytest.raises(RuntimeError):
        s.interpolation_plan(np.zeros((5, 2)))                     # prepare() first
    s.prepare(xi=S, xk=S[hoods])
    dev = torch.device("cuda", 0)
    X_d = torch.from_numpy(rng.uniform(0.0, 1.0, size=(64 + 37, 2))).to(dev)
    plan = s.interpolation_plan(X_d)                                 # prepare() is enough: no prep_interpolate(), no solve
    near = s.interpolation_plan(X_d, mode="continuous", r=0.1)
    fi = np.zeros((n, 6))
    s.solve(fk=np.sin(2.0 * S).prod(axis=1)[hoods], fi=fi)
    fi_d = torch.from_numpy(fi).to(dev)
    want, want_c = plan.evaluate([0, 3], fi=fi_d).clone(), near.evaluate([0, 3], fi=fi_d).clone()
    assert torch.equal(plan.evaluate([0, 3]), want)
    empty = s.interpolation_plan(X_d[:0])                            # nx == 0: a plan of nothing
    assert empty.nx == 0 and empty.evaluate([0, 1], fi=fi_d).shape == (2, 0) and empty.I.shape == (0,)
    s.close()
    assert torch.equal(plan.evaluate([0, 3], fi=fi_d), want)
    with pytest.raises(RuntimeError):
        plan.evaluate(0)                                           # the solver behind fi=None is gone
    del s
    gc.collect()
    assert torch.equal(plan.evaluate([0, 3], fi=fi_d), want)
    assert torch.equal(near.evaluate([0, 3], fi=fi_d).view(torch.int64), want_c.view(torch.int64))
    with pytest.raises(RuntimeError):
        plan.evaluate(0)
    assert plan.memory_used() > 0
    plan.close()
    plan.close()
    with pytest.raises(RuntimeError):
        plan.evaluate(0, fi=fi_d)
    with pytest.raises(RuntimeError):
        plan.memory_used()
