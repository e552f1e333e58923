"""GPU tests of the stacked right-hand sides (wlsqm.hip.StencilSolver(nfields=...): solve_many, enqueue_many, info_many, product_many,
differentiable_stencil_solve_many; csrc/krylov.hip's krylov_*_many kernels).

The statement under test is one: field r of a stacked solve is, BIT FOR BIT, the single-field solver on b_r, x_r alone — x, the iteration
count, the status and the residual, with every preconditioner, forward and transposed.  No comparison here has a tolerance.

  1. identity with single solves, nfields 2, 3, 4, 5, 8 (every pitch, with and without padding fields), one field b = 0 from x = 0, one
     started from a guess, the fields stopping at different iteration counts (asserted: the freeze path runs);
  2. isolation: a NaN in one field's b stays in that field (status 3, x as given); a singular diagonal block is status 4 on every field;
  3. sizes: one row, a slice less one, one slice, two slices, empty rows and an empty slice, and 65 537 rows, where the reduce loops;
  4. strides of b and x; 5. launch-only behaviour and graph capture; 6. autograd with respect to b; 7. refusals.
"""
import numpy as np
import pytest

import _krylov_block_ref as KB
import _krylov_ref as KR
from _device_helpers import bits, dev as _t, nan as _nan, same_bits as _same_bits, wlsqm  # noqa: F401 (fixture)
from test_gpu_krylov import _build

pytestmark = pytest.mark.gpu

SEED = 97
GUESS_FIELD, ZERO_FIELD = 0, 1                                           # field 0 starts from KR.guess(n); field 1 is b = 0 from x = 0
NFIELDS = (2, 3, 4, 5, 8)
CASES = ([(name, pre) for name in ("2D-tau0.25-n130", "2D-dirichlet-n1000", "3D-tau0.25-n1000", "random-n130")
          for pre in ("none", "jacobi", "block16")] + [("2D-tau1-n130", "block8"), ("2D-tau1-n130", "block32")])


def _pre(whip, pre):
    return {"none": None, "jacobi": "jacobi"}[pre] if not pre.startswith("block") else whip.BlockJacobi(int(pre[5:]))


def _cap(name, pre):
    return KB.CAPS[name][int(pre[5:])] if pre.startswith("block") else KR.maxiter(name)


def _field(n, r):
    """(b_r, the start of x_r) of field r, whatever nfields is."""
    b = np.random.default_rng([SEED, r]).standard_normal(n)
    if r == ZERO_FIELD:
        b = np.zeros(n)
    return b, (KR.guess(n) if r == GUESS_FIELD else np.zeros(n))


def _stack(n, nfields):
    fields = [_field(n, r) for r in range(nfields)]
    return _t(np.stack([f[0] for f in fields])), _t(np.stack([f[1] for f in fields]))


_made, _singles = {}, {}


def _system(name):
    """The system `name` on a cloud in Morton order, on the device: built once and left unchanged."""
    if name not in _made:
        import wlsqm.hip as whip
        sy = KB.morton_system(name)
        op, args = _build(whip, sy)
        _made[name] = dict(sy=sy, op=op, args=args, n=sy["n"])
    return _made[name]


def _single(name, pre, transpose, r):
    """(x, SolveInfo) of field r solved alone by a fresh nfields = 1 solver: computed once, shared, left unchanged."""
    key = (name, pre, transpose, r)
    if key not in _singles:
        import wlsqm.hip as whip
        m = _system(name)
        b, x0 = _field(m["n"], r)
        solver = whip.StencilSolver(m["op"], preconditioner=_pre(whip, pre), **m["args"])
        x = _t(x0)
        info = solver.solve(_t(b), x, rtol=KR.RTOL, maxiter=_cap(name, pre), transpose=transpose)
        _singles[key] = (x.cpu().numpy(), info)
        solver.close()
    return _singles[key]


def _same_info(a, b):
    return (a.status, a.iterations) == (b.status, b.iterations) and _same_bits(np.array([a.residual]), np.array([b.residual]))


def _assert_fields_are_the_singles(x, infos, singles, what):
    x = x.cpu().numpy()
    assert len(infos) == len(singles)
    for r, (xs, info_s) in enumerate(singles):
        assert _same_info(infos[r], info_s), (what, r, infos[r], info_s)
        assert _same_bits(x[r], xs), (what, r, "x differs from the single solve", int((x[r] != xs).sum()))


# ---- 1. identity with single solves -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,pre", CASES)
def test_every_field_is_its_single_solve(wlsqm, name, pre):
    import wlsqm.hip as whip
    m = _system(name)
    n, cap = m["n"], _cap(name, pre)
    for nfields in NFIELDS:
        solver = whip.StencilSolver(m["op"], preconditioner=_pre(whip, pre), nfields=nfields, **m["args"])
        assert solver.memory_used() >= wlsqm._binding.lib().wlsqm_hip_krylov_many_workspace_bytes(n, nfields)
        for transpose in (False, True):
            b, x = _stack(n, nfields)
            infos = solver.solve_many(b, x, rtol=KR.RTOL, maxiter=cap, transpose=transpose)
            assert whip.last_kernel() == ("krylov-update-block-many" if pre.startswith("block") else "krylov-update-many")
            singles = [_single(name, pre, transpose, r) for r in range(nfields)]
            what = "%s %s nfields %d%s" % (name, pre, nfields, " transposed" if transpose else "")
            print("%s: iterations %s, statuses %s" % (what, [i.iterations for i in infos], [i.status for i in infos]))
            _assert_fields_are_the_singles(x, infos, singles, what)
            assert infos == solver.info_many()
            assert (infos[ZERO_FIELD].status, infos[ZERO_FIELD].iterations, infos[ZERO_FIELD].residual) == (0, 0, 0.0)
            assert bool((x[ZERO_FIELD] == 0.0).all()) and infos[GUESS_FIELD].iterations > 0
            if (name, nfields) == ("2D-dirichlet-n1000", 8) and pre != "none":
                # the freeze path: fields that converged go on being launched over while the others run
                counts = {i.iterations for i in infos if i.status == 0 and i.iterations > 0}
                assert len(counts) >= 2, (what, [i.iterations for i in infos])
        solver.close()


# ---- 2. isolation --------------------------------------------------------------------------------------------------------------------------

def test_a_nan_stays_in_its_field(wlsqm):
    import wlsqm.hip as whip
    name, nfields, bad = "2D-tau0.25-n130", 4, 2
    m = _system(name)
    n = m["n"]
    for pre in ("jacobi", "block16", "none"):
        solver = whip.StencilSolver(m["op"], preconditioner=_pre(whip, pre), nfields=nfields, **m["args"])
        b, x = _stack(n, nfields)
        b[bad, 3] = float("nan")
        given = KR.guess(n) * 0.5
        x[bad] = _t(given)
        infos = solver.solve_many(b, x, rtol=KR.RTOL, maxiter=_cap(name, pre))
        assert (infos[bad].status, infos[bad].iterations) == (KR.NONFINITE, 0) and _same_bits(x[bad].cpu().numpy(), given), (pre, infos)
        for r in range(nfields):
            if r != bad:
                xs, info_s = _single(name, pre, False, r)
                assert _same_info(infos[r], info_s) and _same_bits(x[r].cpu().numpy(), xs), (pre, r, infos[r], info_s)
        solver.close()


def test_a_singular_block_is_status_4_on_every_field(wlsqm):
    import wlsqm.hip as whip
    st = KB.singular_block_structure()
    n, nfields = st["npoints"], 3
    op = whip.StencilOperator.from_coefficients(_t(st["hoods"]), _t(st["nk"]), _t(st["slots"]), n, own=_t(st["own"]), own_mask=_t(st["own_mask"]))
    b = _t(np.random.default_rng(89).standard_normal((nfields, n)))
    x0 = np.stack([KR.guess(n) * (r + 1) for r in range(nfields)])
    for nb in KB.BLOCKS:
        solver = whip.StencilSolver(op, diag=KB.SINGULAR_DIAG, scale=1.0, preconditioner=whip.BlockJacobi(nb), nfields=nfields)
        x = _t(x0)
        infos = solver.solve_many(b, x)
        assert all((i.status, i.iterations) == (KR.DIAGONAL, 0) for i in infos) and _same_bits(x.cpu().numpy(), x0), (nb, infos)
        solver.enqueue_many(b, x, 5)                                     # what is enqueued behind the stop leaves x alone
        assert all(i.status == KR.DIAGONAL for i in solver.info_many()) and _same_bits(x.cpu().numpy(), x0)
        solver.close()
    op.close()


# ---- 3. sizes -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nrows", (1, 63, 64, 65, 300, 65537))
def test_sizes_product_and_three_iterations(wlsqm, nrows):
    import wlsqm.hip as whip
    st = KR.square_structure(nrows, 9, seed=31)
    if nrows >= 300:
        assert np.all(np.asarray(st["nk"][64:128]) == 0)                 # an empty slice
    op = whip.StencilOperator.from_coefficients(_t(st["hoods"]), _t(st["nk"]), _t(st["slots"]), nrows, own=_t(st["own"]),
                                                own_mask=_t(st["own_mask"]))
    rng = np.random.default_rng([37, nrows])
    d, c = _t(3.0 + rng.random(nrows)), -0.75
    V = rng.standard_normal((8, nrows)) * 10.0 ** rng.integers(-2, 3, (8, nrows))
    Wt = rng.standard_normal((8, nrows))
    Bs = rng.standard_normal((8, nrows))
    one = whip.StencilSolver(op, diag=d, scale=c)
    products = [one.product(_t(V[r]), _t(Wt[r])) for r in range(8)]
    for nfields in (2, 3, 8):
        many = whip.StencilSolver(op, diag=d, scale=c, nfields=nfields)
        out = _nan(nfields, nrows)
        got, dots_w, dots_v = many.product_many(_t(V[:nfields]), _t(Wt[:nfields]), out=out)
        assert got is out and whip.last_kernel() == "krylov-spmv-many"
        for r in range(nfields):
            ref, dw, dv = products[r]
            assert _same_bits(got[r].cpu().numpy(), ref.cpu().numpy()), (nrows, nfields, r)
            assert _same_bits(np.array([dots_w[r], dots_v[r]]), np.array([dw, dv])), (nrows, nfields, r, dots_w[r], dw, dots_v[r], dv)
        many.close()
    one.close()
    for pre in ("jacobi", "block16"):
        one = whip.StencilSolver(op, diag=d, scale=c, preconditioner=_pre(whip, pre))
        refs = []
        for r in range(8):
            x = _t(np.zeros(nrows))
            one.enqueue(_t(Bs[r]), x, 3, rtol=0.0)
            refs.append((x.cpu().numpy(), one.info()))
        for nfields in (2, 3, 8):
            many = whip.StencilSolver(op, diag=d, scale=c, preconditioner=_pre(whip, pre), nfields=nfields)
            x = _t(np.zeros((nfields, nrows)))
            many.enqueue_many(_t(Bs[:nfields]), x, 3, rtol=0.0)
            _assert_fields_are_the_singles(x, many.info_many(), refs[:nfields], "nrows %d %s nfields %d" % (nrows, pre, nfields))
            many.close()
        one.close()
    op.close()


# ---- 4. strides ---------------------------------------------------------------------------------------------------------------------------

def test_strides_of_b_and_x(wlsqm):
    import torch
    import wlsqm.hip as whip
    name, nfields = "2D-tau0.25-n130", 3
    m = _system(name)
    n, cap = m["n"], _cap(name, "jacobi")
    solver = whip.StencilSolver(m["op"], nfields=nfields, **m["args"])
    b0, x0 = _stack(n, nfields)
    singles = [_single(name, "jacobi", False, r) for r in range(nfields)]

    def layouts(t):
        point_major = torch.empty((n, nfields), dtype=torch.float64, device="cuda")
        point_major.copy_(t.T)
        rows = _nan(2 * nfields, n)
        rows[::2] = t
        return t.clone(), point_major.T, rows[::2]

    for b, x in zip(layouts(b0), layouts(x0)):
        assert tuple(b.shape) == tuple(x.shape) == (nfields, n)
        infos = solver.solve_many(b, x, rtol=KR.RTOL, maxiter=cap)
        _assert_fields_are_the_singles(x, infos, singles, "strides %s" % (tuple(x.stride()),))
    # b may repeat one right-hand side (stride 0); x may not
    infos = solver.solve_many(b0[2:3].expand(nfields, n), x0.clone().zero_(), rtol=KR.RTOL, maxiter=cap)
    assert len({(i.status, i.iterations, i.residual) for i in infos}) == 1
    with pytest.raises(ValueError, match="the elements of x must be distinct in memory"):
        solver.solve_many(b0, x0[:1].expand(nfields, n))
    solver.close()


# ---- 5. launch-only behaviour ----------------------------------------------------------------------------------------------------------------

def test_enqueue_behind_the_stop(wlsqm):
    import torch
    import wlsqm.hip as whip
    name, nfields = "2D-dirichlet-n130", 4
    m = _system(name)
    n = m["n"]
    for pre in ("jacobi", "block16"):
        solver = whip.StencilSolver(m["op"], preconditioner=_pre(whip, pre), nfields=nfields, **m["args"])
        b, x = _stack(n, nfields)
        infos = solver.solve_many(b, x, rtol=KR.RTOL, maxiter=_cap(name, pre), check_every=1)
        assert all(i.status == 0 for i in infos)
        k = max(i.iterations for i in infos)
        _, y = _stack(n, nfields)
        before = torch.cuda.memory_allocated()
        solver.enqueue_many(b, y, k + 5, rtol=KR.RTOL)
        assert torch.cuda.memory_allocated() == before
        assert solver.info_many() == infos and torch.equal(bits(y), bits(x))
        solver.close()


def test_capture_behind_update(wlsqm):
    import torch
    import wlsqm.hip as whip
    name, nfields = "2D-tau0.25-n130", 3
    sy = KB.morton_system(name)
    n = sy["n"]
    rng = np.random.default_rng(41)
    SA, SB = sy["S"], sy["S"] + 0.05 * n ** -0.5 * rng.standard_normal(sy["S"].shape)
    S = _t(SA)
    op = whip.StencilOperator(2, 2, S, _t(sy["hoods"]), _t(sy["nk"]), _t(sy["knowns"]), _t(sy["wm"]), _t(sy["rows"]))
    b, x0 = _stack(n, nfields)
    for pre in ("jacobi", "block16"):
        S.copy_(_t(SA))
        solver = whip.StencilSolver(op, diag=sy["diag"], scale=sy["scale"], preconditioner=_pre(whip, pre), nfields=nfields)
        x = _nan(nfields, n)
        iters = 40                                                       # a count to enqueue, not a bound: the solves stop long before

        def step():
            x.copy_(x0)
            op.update(S, check=False)
            solver.enqueue_many(b, x, iters)

        step()                                                           # warm-up outside the capture
        at_a, info_a = x.clone(), solver.info_many()
        S.copy_(_t(SB))
        step()
        eager, info_b = x.clone(), solver.info_many()
        assert all(i.status == 0 for i in info_a + info_b) and not torch.equal(bits(eager), bits(at_a))
        S.copy_(_t(SA))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
            step()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(x), bits(at_a)) and solver.info_many() == info_a
        S.copy_(_t(SB))
        x.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(x), bits(eager)) and solver.info_many() == info_b
        for call, what in ((lambda: solver.solve_many(b, x), "solve_many"), (solver.info_many, "info_many")):
            refused = torch.cuda.CUDAGraph()
            with pytest.raises(RuntimeError, match="%s reads the solve's scalars on the host and the stream is capturing" % what):
                with torch.cuda.graph(refused, stream=torch.cuda.Stream()):
                    call()
            torch.cuda.synchronize()
        solver.close()
    op.close()


# ---- 6. autograd -----------------------------------------------------------------------------------------------------------------------------

def test_gradient_with_respect_to_b(wlsqm):
    import torch
    import wlsqm.hip as whip
    name, nfields = "2D-dirichlet-n130", 3
    m = _system(name)
    n = m["n"]
    b0, _ = _stack(n, nfields)
    b0[ZERO_FIELD] = _t(np.random.default_rng([SEED, 11]).standard_normal(n))
    w = _t(np.random.default_rng([SEED, 13]).standard_normal((nfields, n)))
    many = whip.StencilSolver(m["op"], nfields=nfields, **m["args"])
    b = b0.clone().requires_grad_(True)
    xs = whip.differentiable_stencil_solve_many(many, b, rtol=KR.RTOL)
    (xs * w).sum().backward()
    assert all(i.status == 0 for i in many.info_many())
    one = whip.StencilSolver(m["op"], **m["args"])
    for r in range(nfields):
        br = b0[r].clone().requires_grad_(True)
        xr = whip.differentiable_stencil_solve(one, br, rtol=KR.RTOL)
        (xr * w[r]).sum().backward()
        assert torch.equal(bits(xs[r].detach()), bits(xr.detach())) and torch.equal(bits(b.grad[r]), bits(br.grad)), r
    many.close(); one.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals(wlsqm):
    import torch
    import wlsqm.hip as whip
    m = _system("2D-tau0.25-n130")
    n = m["n"]
    for bad in (0, 9, True, 2.0):
        with pytest.raises(ValueError, match="nfields must be an int, 1 .. 8"):
            whip.StencilSolver(m["op"], nfields=bad, **m["args"])
    solver = whip.StencilSolver(m["op"], nfields=3, **m["args"])
    f64 = dict(dtype=torch.float64, device="cuda")
    b, x, both = torch.ones((3, n), **f64), torch.zeros((3, n), **f64), torch.zeros((6, n), **f64)
    for bad_b, bad_x, message in ((b[:2], x, "b must be a float64 device tensor of shape \\(3, 130\\).*got shape \\(2, 130\\)"),
                                  (b, torch.zeros((4, n), **f64), "x must be a float64 device tensor of shape \\(3, 130\\)"),
                                  (b.float(), x, "expected 'float64'.*argument b"), (b.cpu(), x, "argument b must be a device"),
                                  (b[0], x, "wrong number of dimensions"), (both[:3], both[2:5], "b overlaps x"),
                                  (b, solver._ws[:3 * n].view(3, n), "x overlaps workspace")):
        for call in (solver.solve_many, lambda b_, x_: solver.enqueue_many(b_, x_, 4)):
            with pytest.raises(ValueError, match=message):
                call(bad_b, bad_x)
    for bad_v, bad_out, message in ((b[:2], x, "v must be a float64 device tensor of shape \\(3, 130\\)"), (both[:3], both[2:5], "v overlaps out"),
                                    (b, x[:1].expand(3, n), "the elements of out must be distinct in memory")):
        with pytest.raises(ValueError, match=message):
            solver.product_many(bad_v, out=bad_out)
    assert all(i.status == 0 for i in solver.solve_many(b, x))           # the solver is none the worse
    # nfields = 1 takes the stacked calls too, on the single-field kernels
    one = whip.StencilSolver(m["op"], **m["args"])
    y = torch.zeros((1, n), **f64)
    infos = one.solve_many(b[:1], y)
    assert whip.last_kernel() == "krylov-update" and len(infos) == 1 and infos == one.info_many()
    assert torch.equal(bits(y[0]), bits(x[0]))
    with pytest.raises(ValueError, match="b must be a float64 device tensor of shape \\(1, 130\\)"):
        one.solve_many(b, x)
    solver.close(); one.close()
    with pytest.raises(RuntimeError, match="the stencil solver has been closed"):
        solver.solve_many(b, x)
