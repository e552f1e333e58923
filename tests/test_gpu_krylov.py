"""GPU tests of the implicit solves (wlsqm.hip.StencilSolver, csrc/krylov.hip).

  1. the fused product and the dot products of its pass against exact arithmetic, within bounds that are derived, not measured:
     v within gamma_{len+2} (|d x| + |c| sum |val x|) of the exact row sum; a dot product of n terms within gamma_{n + depth} sum |a_i b_i|,
     depth = 6 + 3 (the wave's tree, the workgroup's waves) + ceil(nwg / 256) + 6 + 3 (the reduce kernel's loop, tree and waves).
     The reduce loops from 257 workgroups on: 65 537 rows is the smallest such size;
  2. solves of the systems of tests/_krylov_ref.py (the rehearsed ones through the real constructor, and a diagonally dominant random
     structure): status 0, iterations within the cap that tests/test_krylov_host.py ties to the reference's count, the true residual
     within max(rtol ||b||, atol) + 8 gap (gap: the reference's own |true - recursive| residual on the same matrix), the error against
     numpy's direct solve within kappa_2(M) times the relative residual;
  3. determinism, the early exit, graph capture behind op.update; 4. statuses, never a fault; 5. refusals.
"""
import math

import numpy as np
import pytest

import _krylov_ref as KR
import _stencil_ref as R
from _device_helpers import bits, dev as _t, nan as _nan, same_bits as _same_bits, wlsqm  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu


def _build(whip, sy):
    """(op, solver arguments): the system on the device."""
    if sy["kind"] == "random":
        st = sy["st"]
        op = whip.StencilOperator.from_coefficients(_t(st["hoods"]), _t(st["nk"]), _t(st["slots"]), sy["n"], own=_t(st["own"]),
                                                    own_mask=_t(st["own_mask"]))
        return op, dict(diag=_t(sy["diag"]), scale=sy["scale"])
    op = whip.StencilOperator(sy["dim"], sy["order"], _t(sy["S"]), _t(sy["hoods"]), _t(sy["nk"]), _t(sy["knowns"]), _t(sy["wm"]), _t(sy["rows"]))
    return op, dict(diag=sy["diag"], scale=sy["scale"])


_made = {}


def _system(name):
    """The system `name` on the device and everything the tests share about it, computed once and left unchanged: dict(sy, op, solver,
    M (dense, from the operator's own values), b (device), xstar, stop)."""
    if name not in _made:
        import wlsqm.hip as whip
        sy = KR.system(name)
        op, args = _build(whip, sy)
        M = KR.dense_of(sy, op.to_sparse_csr(0).to_dense().cpu().numpy())
        _made[name] = dict(sy=sy, op=op, args=args, solver=whip.StencilSolver(op, **args), M=M, b=_t(sy["b"]),
                           xstar=np.linalg.solve(M, sy["b"]), stop=KR.RTOL * np.linalg.norm(sy["b"]), kappa=np.linalg.cond(M))
    return _made[name]


def _held_to_the_reference(m, x, info, x0, dinv, cap, what):
    """The checks of a solve (item 2 of the module's docstring) against the reference run on the same matrix."""
    sy, M = m["sy"], m["M"]
    b = sy["b"]
    xr, its_r, st_r, hist = KR.bicgstab_ref(M, b, x0, dinv, KR.RTOL, 0.0, cap)
    assert st_r == KR.CONVERGED, (what, st_r, its_r)
    gap = abs(np.linalg.norm(b - M @ xr) - hist[-1])
    true = np.linalg.norm(b - M @ x)
    err = np.linalg.norm(x - m["xstar"]) / np.linalg.norm(m["xstar"])
    print("%s: iterations %d (reference %d, cap %d), recursive %.3e true %.3e stop %.3e gap %.3e, error %.3e bound %.3e"
          % (what, info.iterations, its_r, cap, info.residual, true, m["stop"], gap, err, m["kappa"] * true / np.linalg.norm(b)))
    assert info.status == KR.CONVERGED, (what, info)
    assert 0 < info.iterations <= cap, (what, info)
    assert info.residual <= m["stop"]
    assert true <= m["stop"] + 8 * gap, (what, true, m["stop"], gap)
    assert err <= m["kappa"] * true / np.linalg.norm(b) * (1 + 1e-6), (what, err)


# ---- 1. the fused product and its dots ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nrows", (1, 63, 64, 65, 130, 300, 65537))
def test_product_and_dots_against_exact_arithmetic(wlsqm, nrows):
    import torch
    import wlsqm.hip as whip
    from fractions import Fraction
    K, c = 9, -0.75
    st = KR.square_structure(nrows, K, seed=31)
    rows = R.rows_of(st["hoods"], st["nk"], st["slots"], st["own"], st["own_mask"], st["pts"])
    lens = np.array([len(r) for r in rows])
    if nrows >= 130:
        assert lens.min() == 0 and np.all(lens[64:128] == 0)            # empty rows and an empty slice
    rng = np.random.default_rng([37, nrows])
    x = rng.standard_normal(nrows) * 10.0 ** rng.integers(-2, 3, nrows)
    w = rng.standard_normal(nrows)
    d = rng.standard_normal(nrows)
    op = whip.StencilOperator.from_coefficients(_t(st["hoods"]), _t(st["nk"]), _t(st["slots"]), nrows, own=_t(st["own"]),
                                                own_mask=_t(st["own_mask"]))
    m = R.pack(rows, 1)
    assert np.array_equal(op._m["col"].cpu().numpy(), m["col"]) and _same_bits(op._val.cpu().numpy(), m["val"])
    solver = whip.StencilSolver(op, diag=_t(d), scale=c)
    out = _nan(nrows)
    got, dot_w, dot_v = solver.product(_t(x), _t(w), out=out)
    assert whip.last_kernel() == "krylov-spmv-dot"
    v = got.cpu().numpy()
    assert np.isfinite(v).all()
    # the rows that are held to the exact sum: all of them, or the head, the tail and a stretch in the middle of the large case
    check = np.arange(nrows) if nrows <= 300 else np.r_[0:200, 32700:32900, nrows - 200:nrows]
    worst = 0.0
    for i in check:
        terms = [Fraction(c) * Fraction(float(val[0])) * Fraction(float(x[col])) for col, val in rows[i]] + [Fraction(float(d[i])) * Fraction(float(x[i]))]
        exact, mag = float(sum(terms, Fraction(0))), float(sum((abs(t) for t in terms), Fraction(0)))
        bound = R.gamma(lens[i] + 2) * mag
        worst = max(worst, abs(v[i] - exact) / bound)
        assert abs(v[i] - exact) <= bound, (nrows, i, v[i], exact, bound)
    nwg = (nrows + 255) // 256
    depth = 6 + 3 + math.ceil(nwg / 256) + 6 + 3
    worst_dot = 0.0
    for got_dot, other in ((dot_w, w), (dot_v, v)):
        exact, mag = KR.exact_dot(v, other)
        bound = float(R.gamma(nrows + depth)) * float(mag)
        worst_dot = max(worst_dot, abs(Fraction(got_dot) - exact) / Fraction(bound))
        assert abs(Fraction(got_dot) - exact) <= bound, (nrows, got_dot, float(exact), bound)
    print("nrows %d: v at %.3f of its bound, the dots at %.3g of theirs" % (nrows, worst, float(worst_dot)))
    again, dw2, dv2 = solver.product(_t(x), _t(w))
    assert torch.equal(bits(again), bits(got)) and (dw2, dv2) == (dot_w, dot_v)
    solver.close(); op.close()


# ---- 2. solves ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", KR.GPU_SYSTEMS)
def test_solve(wlsqm, name):
    import torch
    m = _system(name)
    n = m["sy"]["n"]
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    info = m["solver"].solve(m["b"], x, rtol=KR.RTOL, maxiter=KR.maxiter(name))
    _held_to_the_reference(m, x.cpu().numpy(), info, np.zeros(n), KR.jacobi(m["M"]), KR.maxiter(name), name)


def test_solve_from_a_guess_and_without_preconditioner(wlsqm):
    import torch
    import wlsqm.hip as whip
    m = _system(KR.FIRST)
    n = m["sy"]["n"]
    x0 = KR.guess(n)
    x = _t(x0)
    info = m["solver"].solve(m["b"], x, rtol=KR.RTOL, maxiter=KR.VARIANTS["guess"], check_every=3)
    _held_to_the_reference(m, x.cpu().numpy(), info, x0, KR.jacobi(m["M"]), KR.VARIANTS["guess"], "from a guess")
    plain = whip.StencilSolver(m["op"], preconditioner=None, **m["args"])
    assert plain.memory_used() == m["solver"].memory_used()
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    info = plain.solve(m["b"], x, rtol=KR.RTOL, maxiter=KR.VARIANTS["plain"])
    _held_to_the_reference(m, x.cpu().numpy(), info, np.zeros(n), None, KR.VARIANTS["plain"], "no preconditioner")
    plain.close()


# ---- 3. determinism and capture ---------------------------------------------------------------------------------------------------------

def test_same_bits_twice_and_behind_the_stop(wlsqm):
    import torch
    m = _system("2D-dirichlet-n130")
    solver, b, n = m["solver"], m["b"], m["sy"]["n"]
    cap = KR.maxiter("2D-dirichlet-n130")
    runs = []
    for check_every in (8, 1):
        x = torch.zeros(n, dtype=torch.float64, device="cuda")
        runs.append((solver.solve(b, x, maxiter=cap, check_every=check_every), x))
    assert runs[0][0] == runs[1][0] and runs[0][0].status == 0
    assert torch.equal(bits(runs[0][1]), bits(runs[1][1]))
    k = runs[1][0].iterations
    # k + 5 iterations enqueued with no host read: the five behind the stop leave x and the scalars alone
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    before = torch.cuda.memory_allocated()
    solver.enqueue(b, x, k + 5)
    assert torch.cuda.memory_allocated() == before
    assert solver.info() == runs[1][0]
    assert torch.equal(bits(x), bits(runs[1][1]))
    # and k - 1 iterations are one too few: the early exit is not what made the two agree
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    solver.enqueue(b, x, k - 1)
    assert solver.info().status == KR.MAXITER and solver.info().iterations == k - 1
    assert not torch.equal(bits(x), bits(runs[1][1]))


def test_capture_behind_update(wlsqm):
    import torch
    import wlsqm.hip as whip
    name = "2D-tau0.25-n130"
    sy = KR.system(name)
    n = sy["n"]
    rng = np.random.default_rng(41)
    SA, SB = sy["S"], sy["S"] + 0.05 * n ** -0.5 * rng.standard_normal(sy["S"].shape)
    S = _t(SA)
    op = whip.StencilOperator(2, 2, S, _t(sy["hoods"]), _t(sy["nk"]), _t(sy["knowns"]), _t(sy["wm"]), _t(sy["rows"]))
    solver = whip.StencilSolver(op, diag=sy["diag"], scale=sy["scale"])
    b, x0 = _t(sy["b"]), _t(KR.guess(n))
    x = _nan(n)
    iters = 2 * KR.maxiter(name)                                         # a count to enqueue, not a bound: the solves stop long before

    def step():
        x.copy_(x0)
        op.update(S, check=False)
        solver.enqueue(b, x, iters)

    step()                                                               # warm-up outside the capture
    at_a, info_a = x.clone(), solver.info()
    S.copy_(_t(SB))
    step()
    eager, info_b = x.clone(), solver.info()
    assert info_a.status == info_b.status == 0 and not torch.equal(bits(eager), bits(at_a))
    S.copy_(_t(SA))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        step()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(x), bits(at_a)) and solver.info() == info_a
    S.copy_(_t(SB))
    x.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(x), bits(eager)) and solver.info() == info_b
    for call, what in ((lambda: solver.solve(b, x), "solve"), (solver.info, "info")):
        refused = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="%s reads the solve's scalars on the host and the stream is capturing" % what):
            with torch.cuda.graph(refused, stream=torch.cuda.Stream()):
                call()
        torch.cuda.synchronize()
    x.copy_(x0)
    assert solver.solve(b, x, maxiter=iters) == info_b and torch.equal(bits(x), bits(eager))      # the captures ended cleanly
    solver.close(); op.close()


# ---- 4. statuses, not faults --------------------------------------------------------------------------------------------------------------

def test_statuses(wlsqm):
    import torch
    import wlsqm.hip as whip
    m = _system("2D-dirichlet-n1000")
    sy, solver, n = m["sy"], m["solver"], m["sy"]["n"]
    zeros = lambda: torch.zeros(n, dtype=torch.float64, device="cuda")
    # b = 0 from x = 0: converged before the first iteration
    x = zeros()
    info = solver.solve(zeros(), x)
    assert (info.status, info.iterations, info.residual) == (0, 0, 0.0) and torch.all(x == 0.0)
    # a NaN in b
    bn = m["b"].clone()
    bn[3] = float("nan")
    x = zeros()
    info = solver.solve(bn, x)
    assert info.status == KR.NONFINITE and info.iterations == 0 and torch.all(x == 0.0)
    # the iteration limit: the reported residual is the true one, within the bar of the solves
    x = zeros()
    info = solver.solve(m["b"], x, maxiter=2)
    xr, its_r, st_r, hist = KR.bicgstab_ref(m["M"], sy["b"], np.zeros(n), KR.jacobi(m["M"]), KR.RTOL, 0.0, 2)
    assert (info.status, info.iterations) == (KR.MAXITER, 2) == (st_r, its_r)
    gap = abs(np.linalg.norm(sy["b"] - m["M"] @ xr) - hist[-1])
    true = np.linalg.norm(sy["b"] - m["M"] @ x.cpu().numpy())
    print("maxiter 2: recursive %.6e true %.6e gap %.3e" % (info.residual, true, gap))
    # both norms are n-term floating sums under a root: gamma_n relative each, whatever the residuals
    assert info.residual > m["stop"] and abs(true - info.residual) <= 8 * gap + 2 * R.gamma(sy["n"]) * true
    # a zero row under Jacobi: found before the first iteration, x untouched; without the preconditioner the same system is no error
    st = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in KR.system("random-n130")["st"].items()}
    st["nk"][5], st["own_mask"][5] = 0, False
    op = whip.StencilOperator.from_coefficients(_t(st["hoods"]), _t(st["nk"]), _t(st["slots"]), 130, own=_t(st["own"]), own_mask=_t(st["own_mask"]))
    zero_row = whip.StencilSolver(op, diag=0.0, scale=1.0)
    b, x0 = _t(KR.system("random-n130")["b"]), KR.guess(130)
    x = _t(x0)
    info = zero_row.solve(b, x)
    assert info.status == KR.DIAGONAL and info.iterations == 0 and _same_bits(x.cpu().numpy(), x0)
    zero_row.close(); op.close()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------------

def test_refusals(wlsqm):
    import torch
    import wlsqm.hip as whip
    st = R.random_structure(130, 150, 9, 2, seed=3)
    dev = lambda **kw: {k: _t(v) for k, v in kw.items()}
    wide = whip.StencilOperator.from_coefficients(_t(st["hoods"]), _t(st["nk"]), _t(st["slots"]), 150, **dev(own=st["own"], own_mask=st["own_mask"],
                                                                                                             point_index=st["pts"]))
    with pytest.raises(ValueError, match="must be square"):
        whip.StencilSolver(wide)
    sq = KR.square_structure(130, 9, seed=5)
    moved = whip.StencilOperator.from_coefficients(_t(sq["hoods"]), _t(sq["nk"]), _t(sq["slots"]), 130,
                                                   **dev(own=sq["own"], own_mask=sq["own_mask"], point_index=np.roll(sq["pts"], 1)))
    with pytest.raises(ValueError, match="point_index must be None or the identity"):
        whip.StencilSolver(moved)
    same = whip.StencilOperator.from_coefficients(_t(sq["hoods"]), _t(sq["nk"]), _t(sq["slots"]), 130,
                                                  **dev(own=sq["own"], own_mask=sq["own_mask"], point_index=sq["pts"]))
    sy = KR.system("2D-tau0.25-n130")
    kn = sy["knowns"].copy()
    kn[::3] = 3                                                          # b_F | b_X: a known derivative
    known = whip.StencilOperator(2, 2, _t(sy["S"]), _t(sy["hoods"]), _t(sy["nk"]), _t(kn), _t(sy["wm"]), _t(sy["rows"]))
    assert known.has_known_derivatives
    with pytest.raises(ValueError, match="their affine term belongs in b"):
        whip.StencilSolver(known)
    solver = whip.StencilSolver(same, diag=2.0)
    n = 130
    f64 = dict(dtype=torch.float64, device="cuda")
    b, x, both = torch.ones(n, **f64), torch.zeros(n, **f64), torch.zeros(2 * n, **f64)
    for bad_b, bad_x, message in ((both[:n], both[n - 1:2 * n - 1], "b overlaps x"), (b.float(), x, "expected 'float64'.*argument b"),
                                  (b.cpu(), x, "argument b must be a device"), (b, both[:n + 1], "x must be a contiguous.*shape \\(130,\\)"),
                                  (both[::2], x, "b must be a contiguous.*strides \\(2,\\)"), (b, x[None], "wrong number of dimensions")):
        for call in (solver.solve, lambda b_, x_: solver.enqueue(b_, x_, 4)):
            with pytest.raises(ValueError, match=message):
                call(bad_b, bad_x)
    assert solver.solve(b, x).status == 0                                # the solver is none the worse
    solver.close()
    with pytest.raises(RuntimeError, match="the stencil solver has been closed"):
        solver.solve(b, x)
    solver = whip.StencilSolver(same)
    same.close()
    with pytest.raises(RuntimeError, match="the stencil operator has been closed"):
        solver.solve(b, x)
    with pytest.raises(RuntimeError, match="the stencil operator has been closed"):
        whip.StencilSolver(same)
    for op in (wide, moved, known):
        op.close()
