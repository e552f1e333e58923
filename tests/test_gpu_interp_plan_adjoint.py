"""The adjoint of interpolation plans on the GPU (csrc/interp_plan.hip; InterpolationPlan.evaluate_adjoint, prepare_adjoint,
wlsqm.hip.differentiable_evaluate) against the numpy statement of tests/_interp_adjoint_ref.py, fed with the plan's
own I / lists, and the rule that the bits of grad_fi are a function of the plan and of the field's g.

Bound (derived, not measured): |got - ref| <= (128 + 4 (n + len_max)) eps A per element, with A the sum of the absolute values of the
element's n terms and len_max the longest list of a contributing point (0 in nearest mode): each term carries a handful of roundings
(monomial, weight, w / W), W is a sum of at most len_max terms, and the sum of n terms adds n eps in any order, the butterfly of the
wave form included.  Every test prints the largest observed ratio before it asserts."""
import numpy as np
import pytest

import _interp_adjoint_ref as R

NX = 3000 + 37                     # 47 full waves and a partial one
NMODELS = 4000
RADIUS = {1: 0.004, 2: 0.03, 3: 0.08}
TOP = {1: 4, 2: 4, 3: 3}


@pytest.fixture(scope="module")
def whip():
    import wlsqm.hip as H
    from wlsqm import _binding
    assert _binding.lib().wlsqm_hip_device_count() >= 1, "no HIP device: the GPU tests need a real MI355X"
    return H


_GEOMETRY = {}


def geometry(dim):
    """4 000 models with per-model orders mixed over 0..4 (3D: 0..3) and NX points of which some lie outside the cloud, one g with every
    diff and one coefficient array per dimension.  Shared by the tests; nothing modifies it."""
    if dim in _GEOMETRY:
        return _GEOMETRY[dim]
    import torch
    rng = np.random.default_rng(50 + dim)
    dev = torch.device("cuda", 0)
    xi = rng.uniform(0.0, 1.0, size=(NMODELS, dim))
    xi[100:107] += 5.0                                               # models that no point uses, in either mode
    x = rng.uniform(-0.2, 1.2, size=(NX, dim))
    order = rng.integers(0, TOP[dim] + 1, size=NMODELS).astype(np.int32)
    max_no = R.NDOF[dim][TOP[dim]]
    g = rng.standard_normal((max_no, NX))
    fi = rng.standard_normal((NMODELS, max_no))
    flat = (lambda a: a[:, 0].copy()) if dim == 1 else (lambda a: a)
    geo = dict(dim=dim, dev=dev, xi=xi, x=x, order=order, max_no=max_no, g=g, fi=fi, no=np.array(R.NDOF[dim])[order],
               xi_d=torch.from_numpy(flat(xi)).to(dev), x_d=torch.from_numpy(flat(x)).to(dev), order_d=torch.from_numpy(order).to(dev),
               g_d=torch.from_numpy(g).to(dev), fi_d=torch.from_numpy(fi).to(dev))
    _GEOMETRY[dim] = geo
    return geo


def make_plan(whip, geo, mode, **kw):
    r = kw.pop("r", RADIUS[geo["dim"]]) if mode == "continuous" else None
    return whip.InterpolationPlan(kw.pop("xi_d", geo["xi_d"]), kw.pop("order_d", geo["order_d"]), kw.pop("x_d", geo["x_d"]), mode=mode, r=r, **kw)


def search_of(plan):
    """What the reference is fed with: the plan's own I or lists."""
    if plan.mode == "nearest":
        return dict(I=plan.I.cpu().numpy())
    off, idx = plan.lists()
    return dict(lists=(off.cpu().numpy(), idx.cpu().numpy()), r=plan.r)


def check(label, got, ref, A, n, len_max):
    """Prints the largest |got - ref| / bound, then asserts the bound element by element."""
    bound = R.bound(A, n, len_max)
    err = np.abs(got - ref)
    live = bound > 0
    worst = float((err[live] / bound[live]).max()) if live.any() else 0.0
    print("%s: largest |got - ref| / bound = %.4f (n up to %d, len_max %d)" % (label, worst, int(n.max()), len_max))
    assert (err <= bound).all(), (label, worst)
    assert (got[~live] == 0.0).all()
    return worst


def bits(t):
    import torch
    return t.contiguous().view(torch.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["nearest", "continuous"])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_every_diff_at_once_against_the_reference(whip, dim, mode):
    """All diffs, one field, into a NaN-filled grad_fi that is wider and taller than [:nmodels, :ncols]: every element of the block is
    written (finite), exact zeros in the columns a model does not have and in unused models' rows, the NaN around it untouched."""
    import torch
    geo = geometry(dim)
    plan = make_plan(whip, geo, mode)
    max_no = geo["max_no"]
    diffs = list(range(max_no))
    buf = torch.full((NMODELS + 5, max_no + 3), float("nan"), dtype=torch.float64, device=geo["dev"])
    ret = plan.evaluate_adjoint(geo["g_d"], diffs, grad_fi=buf)
    assert ret.data_ptr() == buf.data_ptr()
    info = plan.adjoint_info()                                       # (the points outside the cloud crowd on the boundary's models)
    assert whip.last_kernel() == ("interp-plan-adjoint+wave" if info["nlong"] else "interp-plan-adjoint")
    assert info["built"] and info["max_len"] > 0 and info["threshold"] == 64 and (info["nlong"] > 0) == (info["max_len"] > 64)
    got = buf.cpu().numpy()
    block = got[:NMODELS, :max_no]
    assert np.isfinite(block).all()
    assert np.isnan(got[NMODELS:]).all() and np.isnan(got[:, max_no:]).all()
    ref, A, n, len_max = R.adjoint(dim, geo["xi"], geo["order"], geo["x"], geo["g"], diffs, max_no, **search_of(plan))
    assert (len_max > 1) == (mode == "continuous")
    check("dim %d %s" % (dim, mode), block, ref, A, n, len_max)
    beyond = np.arange(max_no)[None, :] >= geo["no"][:, None]
    unused = n.sum(axis=1) == 0
    assert beyond.any() and unused.any() and (~unused).sum() > 500
    assert (block[beyond] == 0.0).all() and (block[unused] == 0.0).all()
    assert (block[~beyond & ~unused[:, None]] != 0.0).any()
    # the default output: allocated, (nmodels, max_no), the same bits
    alone = plan.evaluate_adjoint(geo["g_d"], diffs)
    assert alone.shape == (NMODELS, max_no) and torch.equal(bits(alone), bits(buf[:NMODELS, :max_no]))
    # a wider ncols writes zeros there and nothing beyond
    buf2 = torch.full((NMODELS + 1, max_no + 3), float("nan"), dtype=torch.float64, device=geo["dev"])
    plan.evaluate_adjoint(geo["g_d"], diffs, grad_fi=buf2, ncols=max_no + 2)
    assert torch.equal(bits(buf2[:NMODELS, :max_no]), bits(alone)) and float(buf2[:NMODELS, max_no:max_no + 2].abs().max()) == 0.0
    assert bool(torch.isnan(buf2[:, max_no + 2]).all()) and bool(torch.isnan(buf2[NMODELS]).all())
    with pytest.raises(ValueError):
        plan.evaluate_adjoint(geo["g_d"], diffs, ncols=max_no - 1)
    with pytest.raises(ValueError):
        plan.evaluate_adjoint(geo["g_d"][:, :-1], diffs)
    assert plan.prepare_adjoint() is False                           # the first call built it


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_points_that_do_not_depend_on_fi_are_never_read(whip, dim):
    """Nearest: I with -1 and nmodels.  Continuous: the empty lists, and in 1D one constructed point with W_m == 0 (its only origin at
    distance exactly r, in binary-exact numbers).  g = NaN at all of them: the result is finite and has the bits of a plan built
    without those points."""
    import torch
    geo = geometry(dim)
    max_no, dev = geo["max_no"], geo["dev"]
    diffs = list(range(max_no))
    # nearest
    plan = make_plan(whip, geo, "nearest")
    I = plan.I.clone()
    I[3::194] = -1
    I[100::194] = NMODELS
    dead = (I < 0) | (I >= NMODELS)
    assert int(dead.sum()) > 20
    bad = make_plan(whip, geo, "nearest", I=I)
    g = geo["g_d"].clone()
    g[:, dead] = float("nan")
    got = bad.evaluate_adjoint(g, diffs)
    assert bool(torch.isfinite(got).all())
    keep = ~dead
    kept = make_plan(whip, geo, "nearest", x_d=geo["x_d"][keep].contiguous(), I=I[keep].contiguous())
    want = kept.evaluate_adjoint(geo["g_d"][:, keep].contiguous(), diffs)
    assert torch.equal(bits(got), bits(want))
    # continuous: empty lists (and the W == 0 point in 1D)
    if dim == 1:
        # origin NMODELS sits at -8 with every other origin and point far from it; the point at -8 + 2^-8 is exactly r = 2^-8 away
        # (binary-exact numbers: d2 == r2, t == 0, w == 0, W == 0), and r stays near RADIUS[1] so that no model's list grows long
        r = 2.0 ** -8
        xi_d = torch.cat([geo["xi_d"], torch.tensor([-8.0], dtype=torch.float64, device=dev)])
        order_d = torch.cat([geo["order_d"], torch.tensor([2], dtype=torch.int32, device=dev)])
        x_d = torch.cat([geo["x_d"], torch.tensor([-8.0 + r], dtype=torch.float64, device=dev)])
        g_all = torch.cat([geo["g_d"], torch.ones((max_no, 1), dtype=torch.float64, device=dev)], dim=1)
    else:
        xi_d, order_d, x_d, r, g_all = geo["xi_d"], geo["order_d"], geo["x_d"], RADIUS[dim], geo["g_d"]
    cont = whip.InterpolationPlan(xi_d, order_d, x_d, mode="continuous", r=r)
    value = cont.evaluate(0, fi=torch.ones((xi_d.shape[0], max_no), dtype=torch.float64, device=dev))
    dead = torch.isnan(value)                                        # empty lists and 0 / 0
    off, idx = cont.lists()
    empty = (off[1:] - off[:-1]) == 0
    assert int(empty.sum()) > 20 and bool(dead[empty].all())
    if dim == 1:
        assert bool(dead[-1]) and not bool(empty[-1]) and int(idx[off[-2]:off[-1]][0]) == NMODELS      # W == 0, one origin in the list
    g = g_all.clone()
    g[:, dead] = float("nan")
    got = cont.evaluate_adjoint(g, diffs)
    assert bool(torch.isfinite(got).all())
    if dim == 1:
        assert float(got[NMODELS].abs().max()) == 0.0
    keep = ~dead
    kept = whip.InterpolationPlan(xi_d, order_d, x_d[keep].contiguous(), mode="continuous", r=r)
    want = kept.evaluate_adjoint(g_all[:, keep].contiguous(), diffs)
    assert cont.adjoint_info()["nlong"] == 0                         # (the wave form's order depends on the length of the list)
    assert torch.equal(bits(got), bits(want))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["nearest", "continuous"])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_dot_product_identity_on_the_device(whip, dim, mode):
    """<evaluate(fi), g> == <fi, evaluate_adjoint(g)> for a stack of 3 fields: both sides are sums of the same terms, each side within
    sum (128 + 4 (n + len_max)) eps A |fi| of the exact sum.  The two inner products themselves are taken in long double."""
    import torch
    geo = geometry(dim)
    plan = make_plan(whip, geo, mode)
    max_no = geo["max_no"]
    rng = np.random.default_rng(7 + dim)
    diffs = [0, max_no - 1, 1 % max_no]
    fi = rng.standard_normal((3, NMODELS, max_no))
    g = rng.standard_normal((3, len(diffs), NX))
    out = plan.evaluate(diffs, fi=torch.from_numpy(fi).to(geo["dev"])).cpu().numpy()
    grad = plan.evaluate_adjoint(torch.from_numpy(g).to(geo["dev"]), diffs).cpu().numpy()
    assert out.shape == g.shape and grad.shape == fi.shape
    live = ~np.isnan(out)                                            # NaN where the value does not depend on fi
    assert live.any() and (mode == "nearest") == live.all()
    search = search_of(plan)
    for f in range(3):
        lhs = (out[f][live[f]].astype(np.longdouble) * g[f][live[f]]).sum()
        rhs = (grad[f].astype(np.longdouble) * fi[f]).sum()
        _, A, n, len_max = R.adjoint(dim, geo["xi"], geo["order"], geo["x"], np.where(live[f], g[f], 0.0), diffs, max_no, **search)
        tol = 2.0 * float((R.bound(A, n, len_max) * np.abs(fi[f])).sum())
        print("dim %d %s field %d: |<Jf, g> - <f, J'g>| / bound = %.4f" % (dim, mode, f, abs(float(lhs - rhs)) / tol))
        assert abs(float(lhs - rhs)) <= tol


@pytest.mark.gpu
def test_long_lists_take_the_wave_form_nearest(whip):
    """The caller's I sends exactly T - 1, T, T + 1, 3 T + 5 and 1 000 points to five models: the last three are long."""
    import torch
    geo = geometry(2)
    T = make_plan(whip, geo, "nearest").adjoint_info()["threshold"]
    counts = {7: T - 1, 1900: T, 33: T + 1, 3999: 3 * T + 5, 2500: 1000}
    rng = np.random.default_rng(41)
    I = 200 + np.arange(NX, dtype=np.int64) % 1500                   # two or three points on each of models 200 .. 1699, none on the five
    slots = rng.permutation(NX)
    at = 0
    for model, c in counts.items():
        I[slots[at:at + c]] = model
        at += c
    assert at < NX
    plan = make_plan(whip, geo, "nearest", I=torch.from_numpy(I).to(geo["dev"]))
    diffs = list(range(geo["max_no"]))
    got = plan.evaluate_adjoint(geo["g_d"], diffs).cpu().numpy()
    assert whip.last_kernel() == "interp-plan-adjoint+wave"
    info = plan.adjoint_info()
    assert info["nlong"] == 3 and info["max_len"] == 1000 and info["nentries"] == NX and info["threshold"] == T
    ref, A, n, len_max = R.adjoint(2, geo["xi"], geo["order"], geo["x"], geo["g"], diffs, geo["max_no"], I=I)
    for model, c in counts.items():
        assert n[model, 0] == c
    check("nearest, long lists", got, ref, A, n, len_max)
    toff, tpt = (t.cpu().numpy() for t in plan.transposed_lists())
    assert toff[0] == 0 and toff[-1] == len(tpt) == NX and (np.diff(toff) == np.bincount(I, minlength=NMODELS)).all()
    for i in list(counts) + [200, 0, 1699]:
        mine = tpt[toff[i]:toff[i + 1]]
        assert (np.diff(mine) > 0).all() and np.array_equal(mine, np.nonzero(I == i)[0])
    assert np.array_equal(np.sort(tpt), np.arange(NX)) and (I[tpt] == np.repeat(np.arange(NMODELS), np.diff(toff))).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_long_lists_take_the_wave_form_continuous(whip, dim):
    """40 models and an r that gives every one of them more than T points."""
    import torch
    geo = geometry(dim)
    r = {1: 0.2, 2: 0.45, 3: 0.7}[dim]
    nm = 40
    plan = make_plan(whip, geo, "continuous", r=r, xi_d=geo["xi_d"][:nm].contiguous(), order_d=geo["order_d"][:nm].contiguous())
    diffs = list(range(geo["max_no"]))
    got = plan.evaluate_adjoint(geo["g_d"], diffs).cpu().numpy()
    assert whip.last_kernel() == "interp-plan-adjoint+wave"
    info = plan.adjoint_info()
    off, idx = (t.cpu().numpy() for t in plan.lists())
    per_model = np.bincount(idx, minlength=nm)
    assert per_model.min() > info["threshold"] and info["nlong"] == nm and info["max_len"] == per_model.max() and info["nentries"] == len(idx)
    ref, A, n, len_max = R.adjoint(dim, geo["xi"][:nm], geo["order"][:nm], geo["x"], geo["g"], diffs, geo["max_no"], lists=(off, idx), r=r)
    check("dim %d continuous, long lists" % dim, got, ref, A, n, len_max)
    toff, tpt = (t.cpu().numpy() for t in plan.transposed_lists())
    assert np.array_equal(np.diff(toff), per_model)
    pt = np.repeat(np.arange(NX), np.diff(off))
    for i in range(nm):
        mine = tpt[toff[i]:toff[i + 1]]
        assert (np.diff(mine) > 0).all() and np.array_equal(mine, np.sort(pt[idx == i]))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["nearest", "continuous"])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_the_bits_are_a_function_of_the_plan_and_the_fields_g(whip, dim, mode):
    import torch
    geo = geometry(dim)
    plan = make_plan(whip, geo, mode)
    max_no, dev = geo["max_no"], geo["dev"]
    diffs = list(range(max_no))
    first = plan.evaluate_adjoint(geo["g_d"], diffs)
    assert torch.equal(bits(first), bits(plan.evaluate_adjoint(geo["g_d"], diffs)))              # run to run
    # alone, and as member 1 of a strided stack of 3
    rng = np.random.default_rng(3)
    wide = torch.from_numpy(rng.standard_normal((3, max_no + 2, NX + 9))).to(dev)
    wide[1, 1:1 + max_no, :NX] = geo["g_d"]
    stack_g = wide[:, 1:1 + max_no, :NX]
    assert not stack_g.is_contiguous()
    out = torch.full((3, NMODELS + 2, max_no + 1), float("nan"), dtype=torch.float64, device=dev)
    plan.evaluate_adjoint(stack_g, diffs, grad_fi=out)
    assert torch.equal(bits(out[1, :NMODELS, :max_no]), bits(first))
    assert bool(torch.isfinite(out[:, :NMODELS, :max_no]).all()) and bool(torch.isnan(out[:, NMODELS:]).all()) and bool(torch.isnan(out[:, :, max_no:]).all())
    for f in (0, 2):
        assert torch.equal(bits(out[f, :NMODELS, :max_no]), bits(plan.evaluate_adjoint(stack_g[f], diffs)))
    # the diffs permuted, g permuted alike
    perm = [int(p) for p in np.random.default_rng(9).permutation(max_no)]
    assert torch.equal(bits(plan.evaluate_adjoint(geo["g_d"][perm].contiguous(), perm)), bits(first))
    # a single int diff, g of shape (nx,)
    one = plan.evaluate_adjoint(geo["g_d"][1 % max_no], 1 % max_no)
    assert torch.equal(bits(one), bits(plan.evaluate_adjoint(geo["g_d"][[1 % max_no]], [1 % max_no])))
    # a diff given twice contributes twice; one that nobody has contributes nothing and its g is not read
    d = 2 % max_no
    twice = [d, d, max_no + 3, -1]
    g2 = torch.from_numpy(rng.standard_normal((4, NX))).to(dev)
    g2[2:] = float("nan")
    got = plan.evaluate_adjoint(g2, twice).cpu().numpy()
    assert np.isfinite(got).all()
    ref, A, n, len_max = R.adjoint(dim, geo["xi"], geo["order"], geo["x"], np.nan_to_num(g2.cpu().numpy()), twice, max_no, **search_of(plan))
    check("dim %d %s diff [%d, %d]" % (dim, mode, d, d), got, ref, A, n, len_max)
    # two plans of the same inputs hold identical transposed lists
    a, b = plan.transposed_lists(), make_plan(whip, geo, mode).transposed_lists()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[1].dtype == torch.int64 and a[0].shape == (NMODELS + 1,)


_SOLVER = {}


def solver_problem():
    """A prepared 2D order-2 ExpertSolver on 2 000 points, a plan at 613 off-cloud points (index ready) and fixed random tensors."""
    if _SOLVER:
        return _SOLVER
    import scipy.spatial
    import torch
    import wlsqm
    n, k = 2000, 16
    rng = np.random.default_rng(11)
    S = rng.uniform(0.0, 1.0, size=(n, 2))
    _, hoods = scipy.spatial.cKDTree(S).query(S, k + 1)
    hoods = hoods[:, 1:]
    dev = torch.device("cuda", 0)
    s = wlsqm.ExpertSolver(dimension=2, nk=np.full(n, k, np.int32), order=np.full(n, 2, np.int32),
                           knowns=np.zeros(n, np.int64), weighting_method=np.full(n, wlsqm.WEIGHT_CENTER, np.int32))
    s.prepare(xi=S, xk=S[hoods])
    X_d = torch.from_numpy(rng.uniform(0.0, 1.0, size=(64 * 9 + 37, 2))).to(dev)
    _SOLVER.update(n=n, k=k, dev=dev, solver=s, X_d=X_d, nx=int(X_d.shape[0]), rng=rng,
                   fk=torch.from_numpy(rng.standard_normal((n, k))).to(dev),
                   g=torch.from_numpy(rng.standard_normal((3, int(X_d.shape[0])))).to(dev))
    return _SOLVER


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["nearest", "continuous"])
def test_autograd(whip, mode):
    import torch
    p = solver_problem()
    s, dev, n, nx = p["solver"], p["dev"], p["n"], p["nx"]
    plan = s.interpolation_plan(p["X_d"], mode=mode, r=0.08 if mode == "continuous" else None)
    diffs = [0, 1, 2]
    g = p["g"]
    # fi taller and wider than needed: the forward's bits, the adjoint's bits, zeros around them
    fi = torch.from_numpy(np.random.default_rng(5).standard_normal((n + 3, 8))).to(dev).requires_grad_(True)
    out = whip.differentiable_evaluate(plan, fi, diffs)
    assert out.grad_fn is not None
    plain = plan.evaluate(diffs, fi=fi.detach())
    assert plain.grad_fn is None and torch.equal(bits(torch.nan_to_num(out.detach(), nan=-3.0)), bits(torch.nan_to_num(plain, nan=-3.0)))
    live = ~torch.isnan(plain)
    gl = torch.where(live, g, torch.zeros_like(g))
    (torch.where(live, out, torch.zeros_like(out)) * gl).sum().backward()
    want = plan.evaluate_adjoint(gl, diffs)
    assert fi.grad.shape == fi.shape and torch.equal(bits(fi.grad[:n, :6]), bits(want))
    assert float(fi.grad[n:].abs().max()) == 0.0 and float(fi.grad[:, 6:].abs().max()) == 0.0 and float(fi.grad.abs().max()) > 0.0
    # chained behind differentiable_solve: fk.grad has the bits of solve_adjoint_device(evaluate_adjoint(g))
    fk = p["fk"].clone().requires_grad_(True)
    fi0 = torch.zeros((n, 6), dtype=torch.float64, device=dev)

    def loss(fk_t):
        val = whip.differentiable_evaluate(plan, whip.differentiable_solve(s, fk_t, fi0), diffs)
        return (torch.where(live, val, torch.zeros_like(val)) * gl).sum()

    L0 = loss(fk)
    L0.backward()
    gfk, _ = s.solve_adjoint_device(plan.evaluate_adjoint(gl, diffs))
    assert torch.equal(bits(fk.grad), bits(gfk))
    # the map fk -> L is linear: L(fk + v) - L(fk) == <fk.grad, v> up to the rounding of the three sums.  Each of L(fk + v), L(fk) and
    # the inner product is a sum of products whose absolute values add up to at most S = <|val|, |g|> resp. <|grad|, |v|>; the solve
    # behind val is accurate to about cond * eps, covered by the factor 1e4 on eps * S.
    v = torch.from_numpy(np.random.default_rng(6).standard_normal((n, p["k"]))).to(dev)
    with torch.no_grad():
        L1 = loss(fk.detach() + v)
        val1 = plan.evaluate(diffs, fi=_solved(s, fk.detach() + v, fi0))
        scale = float((torch.nan_to_num(val1).abs() * gl.abs()).sum() + (fk.grad.abs() * v.abs()).sum() + abs(float(L0)))
    lhs, rhs = float(L1 - L0), float((fk.grad * v).sum())
    print("%s: L(fk + v) - L(fk) = %.15e, <grad, v> = %.15e, |difference| / (eps S) = %.2f" % (mode, lhs, rhs, abs(lhs - rhs) / (R.EPS * scale)))
    assert abs(lhs - rhs) <= 1e4 * R.EPS * scale
    # no gradient asked for: nothing is computed, and the geometry has none to give
    assert whip.differentiable_evaluate(plan, fi.detach(), 0).grad_fn is None
    with pytest.raises(ValueError, match="not differentiable"):
        whip.differentiable_evaluate(s.interpolation_plan(p["X_d"].clone().requires_grad_(True)), fi)
    xi_d = torch.from_numpy(np.random.default_rng(8).uniform(size=(50, 2))).to(dev)
    with pytest.raises(ValueError, match="not differentiable"):
        whip.differentiable_evaluate(whip.InterpolationPlan(xi_d.clone().requires_grad_(True), 2, p["X_d"]), fi)
    with pytest.raises(ValueError, match="not differentiable"):
        whip.differentiable_evaluate(whip.InterpolationPlan(xi_d, 2, p["X_d"].clone().requires_grad_(True)), fi)


def _solved(s, fk, fi0):
    fi = fi0.clone()
    s.solve_device(fk, fi)
    return fi


@pytest.mark.gpu
def test_solve_evaluate_and_adjoint_replay_from_one_graph(whip):
    """After prepare_adjoint(): solve_device -> evaluate -> evaluate_adjoint captured on one stream in one graph and replayed twice with
    new fk; each replay gives the bits of the eager sequence."""
    import torch
    p = solver_problem()
    s, dev, n, nx = p["solver"], p["dev"], p["n"], p["nx"]
    plan = s.interpolation_plan(p["X_d"])
    assert plan.adjoint_info() == dict(built=False, nentries=None, max_len=None, nlong=None, threshold=64)
    before = plan.memory_used()
    assert plan.prepare_adjoint() is True and plan.prepare_adjoint() is False
    assert plan.adjoint_info()["built"] and plan.memory_used() > before
    diffs = [0, 1, 2]
    fk = torch.empty((n, p["k"]), dtype=torch.float64, device=dev)
    fi = torch.zeros((n, 6), dtype=torch.float64, device=dev)
    val = torch.zeros((3, nx), dtype=torch.float64, device=dev)
    grad = torch.zeros((n, 6), dtype=torch.float64, device=dev)

    def step():
        s.solve_device(fk, fi)
        plan.evaluate(diffs, fi=fi, out=val)
        plan.evaluate_adjoint(val, diffs, grad_fi=grad)              # the gradient of 0.5 |values|^2

    fk.copy_(p["fk"])
    step()                                                           # warm-up outside the capture
    torch.cuda.synchronize()
    grad.fill_(-7.0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        step()
    torch.cuda.synchronize()
    assert float(grad.min()) == -7.0 and float(grad.max()) == -7.0   # captured, not run
    rng = np.random.default_rng(12)
    for _ in range(2):
        fk.copy_(torch.from_numpy(rng.standard_normal((n, p["k"]))).to(dev))
        graph.replay()
        torch.cuda.synchronize()
        got_val, got_grad = val.clone(), grad.clone()
        grad.fill_(-7.0); val.fill_(-7.0)
        step()
        torch.cuda.synchronize()
        assert torch.equal(bits(got_val), bits(val)) and torch.equal(bits(got_grad), bits(grad))
        assert float(got_grad.abs().max()) > 0.0


@pytest.mark.gpu
def test_degenerate_sizes(whip):
    import torch
    geo = geometry(2)
    dev, max_no = geo["dev"], geo["max_no"]
    # nx == 0: the adjoint of nothing is zero
    empty = make_plan(whip, geo, "nearest", x_d=geo["x_d"][:0])
    out = torch.full((NMODELS, max_no), float("nan"), dtype=torch.float64, device=dev)
    empty.evaluate_adjoint(torch.zeros((2, 0), dtype=torch.float64, device=dev), [0, 1], grad_fi=out)
    assert float(out.abs().max()) == 0.0
    assert empty.adjoint_info()["nentries"] == 0 and empty.transposed_lists()[1].shape == (0,)
    empty_c = make_plan(whip, geo, "continuous", x_d=geo["x_d"][:0])
    assert float(empty_c.evaluate_adjoint(torch.zeros((0,), dtype=torch.float64, device=dev), 0).abs().max()) == 0.0
    # ndiff == 0
    for mode in ("nearest", "continuous"):
        plan = make_plan(whip, geo, mode)
        out.fill_(float("nan"))
        plan.evaluate_adjoint(torch.zeros((0, NX), dtype=torch.float64, device=dev), [], grad_fi=out)
        assert float(out.abs().max()) == 0.0
    # one model, every point on it: the wave form
    one = whip.InterpolationPlan(geo["xi_d"][:1].contiguous(), 4, geo["x_d"])
    got = one.evaluate_adjoint(geo["g_d"], list(range(max_no))).cpu().numpy()
    assert whip.last_kernel() == "interp-plan-adjoint+wave"
    assert one.adjoint_info() == dict(built=True, nentries=NX, max_len=NX, nlong=1, threshold=64)
    ref, A, n, len_max = R.adjoint(2, geo["xi"][:1], np.array([4]), geo["x"], geo["g"], list(range(max_no)), max_no, I=np.zeros(NX, np.int64))
    assert n.min() == NX
    check("one model, %d points" % NX, got, ref, A, n, len_max)
