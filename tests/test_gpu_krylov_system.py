"""GPU tests of the coupled solves (wlsqm.hip.StencilSystemSolver, csrc/krylov.hip).

  1. the fused product and the dot products of its pass against exact arithmetic, within the bounds that tests/test_gpu_krylov.py holds
     StencilSolver.product to: an unknown of T terms (T = m nop len + m: coupling * val * x per entry, component and plane, and the m
     of the diagonal block) within gamma_{T + 2} of the sum of their magnitudes; a dot product of m n terms within gamma_{m n + depth}
     sum |a_i b_i|, depth = (m - 1) + 6 + 3 + ceil(nwg / 256) + 6 + 3 (the lane's m terms, the wave's tree, the workgroup's waves, the
     reduce kernel's loop, tree and waves), nwg = ceil(n / 256).  At the small sizes the bits are those of the stated order of
     operations (tests/_krylov_system_ref.product_statement).  65 537 points: more than 256 partials for the reduce;
  2. solves of the systems of tests/_krylov_system_ref.py by section 17's criteria against _krylov_ref.bicgstab_ref on the dense M of the
     operator's own values: status 0 within the cap, the recursive residual under the stop, the true residual within
     max(rtol ||b||, atol) + 8 gap (gap: the reference's own |true - recursive| on the same matrix), the error against numpy's direct
     solve within kappa_2(M) times the relative residual;
  3. bit for bit: twice, check_every=1 against one enqueue, eager against a captured op.update + enqueue, a changed diag tensor;
  4. statuses, never a fault; 5. a StencilSolver at work beside it is not disturbed."""
import math
from fractions import Fraction

import numpy as np
import pytest

import _krylov_ref as KR
import _krylov_system_ref as SR
import _stencil_ref as R
from _device_helpers import bits, dev as _t, nan as _nan, same_bits as _same_bits, wlsqm  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

PAIRS = [(1, 1), (2, 3), (3, 4), (4, 7)]
FORMS = ("float", "constants", "tensor")
PRODUCT_CASES = ([(n, m, nop, FORMS[(k + m + nop) % 3]) for k, n in enumerate((65, 300)) for m in (1, 2, 3, 4) for nop in (1, 3, 4, 7)]
                 + [(n, m, nop, FORMS[(k + j) % 3]) for k, n in enumerate((1, 63, 64, 257)) for j, (m, nop) in enumerate(PAIRS)]
                 + [(65537, 1, 3, "tensor"), (65537, 2, 4, "constants"), (65537, 3, 7, "tensor"), (65537, 4, 1, "float")])


def _operator(whip, st):
    return whip.StencilOperator.from_coefficients(_t(st["hoods"]), _t(st["nk"]), _t(st["slots"]), st["npoints"], own=_t(st["own"]),
                                                  own_mask=_t(st["own_mask"]))


def _diag(form, m, n, rng):
    """(what the solver takes, the reference's view) of a diag of the given form."""
    if form == "float":
        return 0.75, 0.75
    if form == "constants":
        d = rng.standard_normal((m, m))
        return d, d
    d = rng.standard_normal((m, m, n))
    return _t(d), d


# ---- 1. the fused product and its dots ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nrows,m,nop,form", PRODUCT_CASES)
def test_product_and_dots_against_exact_arithmetic(wlsqm, nrows, m, nop, form):
    import torch
    import wlsqm.hip as whip
    st = SR.planes_structure(nrows, 9, nop, seed=31)
    rows = SR.rows_of_structure(st)
    lens = np.array([len(r) for r in rows])
    if nrows >= 130:
        assert lens.min() == 0 and np.all(lens[64:128] == 0)            # empty rows and an empty slice
    assert any(len({c for c, _ in r}) < len(r) for r in rows) and any(any(c == i for c, _ in r) for i, r in enumerate(rows))
    rng = np.random.default_rng([37, nrows, m, nop])
    coupling = rng.standard_normal((m, m, nop))
    x = rng.standard_normal((nrows, m)) * 10.0 ** rng.integers(-2, 3, (nrows, m))
    w = rng.standard_normal((nrows, m))
    held, d = _diag(form, m, nrows, rng)
    op = _operator(whip, st)
    solver = whip.StencilSystemSolver(op, coupling, diag=held)
    out = _nan(nrows, m)
    got, dot_w, dot_v = solver.product(_t(x), _t(w), out=out)
    assert got is out and whip.last_kernel() == "krylov-system-spmv"
    v = got.cpu().numpy()
    assert np.isfinite(v).all()
    check = np.arange(nrows) if nrows <= 300 else np.r_[0:40, 32750:32790, nrows - 40:nrows]
    exact, mag = SR.exact_product(rows, coupling, d, x, check)
    bound = R.gamma(m * nop * lens[check] + m + 2)[:, None] * mag
    err = np.abs(v[check] - exact)
    assert np.all(err <= bound), (nrows, m, nop, form, float((err / np.maximum(bound, 1e-300)).max()))
    if nrows <= 65:
        assert _same_bits(v, SR.product_statement(rows, coupling, d, x))
    nwg = (nrows + 255) // 256
    depth = (m - 1) + 6 + 3 + math.ceil(nwg / 256) + 6 + 3
    worst_dot = 0.0
    for got_dot, other in ((dot_w, w), (dot_v, v)):
        ex, mg = KR.exact_dot(v, other)
        bnd = float(R.gamma(m * nrows + depth)) * float(mg)
        worst_dot = max(worst_dot, float(abs(Fraction(got_dot) - ex) / Fraction(bnd)))
        assert abs(Fraction(got_dot) - ex) <= bnd, (nrows, m, nop, got_dot, float(ex), bnd)
    print("n %d m %d nop %d %s: v at %.3f of its bound, the dots at %.3g of theirs" % (nrows, m, nop, form, float((err / np.maximum(bound, 1e-300)).max()), worst_dot))
    again, dw2, dv2 = solver.product(_t(x), _t(w))
    assert torch.equal(bits(again), bits(got)) and (dw2, dv2) == (dot_w, dot_v)
    same, dv3, dv4 = solver.product(_t(x))                                # w defaults to v
    assert torch.equal(bits(same), bits(got)) and dv4 == dot_v
    solver.close(); op.close()


@pytest.mark.parametrize("m,nop", PAIRS)
def test_uncoupled_product_is_the_operators_apply(wlsqm, m, nop):
    """A coupling that is zero off the diagonal: component a is sum_o coupling[a, a, o] op.apply(v[:, a])[o] + d v[:, a], within the
    product's own bound (the terms of that sum: nop per entry and one of d)."""
    import wlsqm.hip as whip
    n, d = 300, -1.25
    st = SR.planes_structure(n, 9, nop, seed=43)
    rows = SR.rows_of_structure(st)
    lens = np.array([len(r) for r in rows])
    rng = np.random.default_rng([47, m])
    coupling = np.zeros((m, m, nop))
    for a in range(m):
        coupling[a, a] = rng.standard_normal(nop)
    x = rng.standard_normal((n, m))
    op = _operator(whip, st)
    solver = whip.StencilSystemSolver(op, coupling, diag=d)
    v = solver.product(_t(x))[0].cpu().numpy()
    exact, mag = SR.exact_product(rows, coupling, d, x)
    bound = R.gamma(nop * lens + 1 + 2)[:, None] * mag
    for a in range(m):
        applied = op.apply(_t(np.ascontiguousarray(x[:, a]))).cpu().numpy()            # (nop, n)
        want = (coupling[a, a][:, None] * applied).sum(axis=0) + d * x[:, a]
        assert np.all(np.abs(v[:, a] - want) <= bound[:, a]), (m, nop, a)
    solver.close(); op.close()


# ---- 2. solves ----------------------------------------------------------------------------------------------------------------------------

_made = {}


def _system(name):
    """The system `name` on the device and what the tests share about it, computed once and left unchanged."""
    if name not in _made:
        import wlsqm.hip as whip
        sy = SR.system(name)
        if sy["kind"] == "random":
            op = _operator(whip, sy["st"])
        else:
            op = whip.StencilOperator(sy["dim"], sy["order"], _t(sy["S"]), _t(sy["hoods"]), _t(sy["nk"]), _t(sy["knowns"]), _t(sy["wm"]),
                                      _t(sy["rows"]))
        diag = _t(sy["diag"]) if np.ndim(sy["diag"]) == 3 else sy["diag"]
        A = np.stack([op.to_sparse_csr(o).to_dense().cpu().numpy() for o in range(sy["nop"])])
        M = SR.dense_matrix(A, sy["coupling"], sy["diag"])
        b = sy["b"].reshape(-1)
        _made[name] = dict(sy=sy, op=op, diag=diag, M=M, b=_t(sy["b"]), bflat=b, xstar=np.linalg.solve(M, b),
                           stop=KR.RTOL * np.linalg.norm(b), kappa=np.linalg.cond(M), solvers={})
    return _made[name]


def _solver(m, pc):
    import wlsqm.hip as whip
    if pc not in m["solvers"]:
        m["solvers"][pc] = whip.StencilSystemSolver(m["op"], m["sy"]["coupling"], diag=m["diag"], preconditioner=pc)
    return m["solvers"][pc]


def _held_to_the_reference(m, x, info, x0, pc, cap, what):
    """Section 17's criteria against the reference run on the same matrix; x and x0 flat."""
    M, b = m["M"], m["bflat"]
    xr, its_r, st_r, hist = SR.solve_ref(M, b, pc, cap=cap, x0=x0)
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


@pytest.mark.parametrize("name,pc", SR.GPU_CASES)
def test_solve(wlsqm, name, pc):
    m = _system(name)
    solver = _solver(m, pc)
    cap = SR.CAPS[name][pc]
    info = solver.solve(m["b"], rtol=KR.RTOL, maxiter=cap)               # x0=None: from zero, in a new tensor
    x = solver.x
    assert tuple(x.shape) == (m["sy"]["n"], m["sy"]["m"])
    _held_to_the_reference(m, x.cpu().numpy().reshape(-1), info, None, pc, cap, "%s %s" % (name, pc))


def test_solve_from_a_guess(wlsqm):
    """A non-zero x0 on a system with a per-point diag tensor and on an elasticity system; the cap is the zero start's (a random start
    of unit size is no further from the solution than zero is, in these systems' norms, by more than the cap's factor of two)."""
    for name in ("random-m3", "elasticity-2D-n130"):
        m = _system(name)
        sy = m["sy"]
        x0 = np.random.default_rng([67, sy["n"]]).standard_normal((sy["n"], sy["m"]))
        x = _t(x0)
        cap = SR.CAPS[name]["jacobi"]
        info = _solver(m, "jacobi").solve(m["b"], x, rtol=KR.RTOL, maxiter=cap, check_every=3)
        assert _solver(m, "jacobi").x is x
        _held_to_the_reference(m, x.cpu().numpy().reshape(-1), info, x0.reshape(-1), "jacobi", cap, name + " from a guess")


# ---- 3. bit for bit -------------------------------------------------------------------------------------------------------------------------

def test_same_bits_twice_and_behind_the_stop(wlsqm):
    import torch
    name = "elasticity-2D-n130"
    m = _system(name)
    solver, b, sy = _solver(m, "jacobi"), m["b"], m["sy"]
    cap = SR.CAPS[name]["jacobi"]
    zeros = lambda: torch.zeros((sy["n"], sy["m"]), dtype=torch.float64, device="cuda")
    runs = []
    for check_every in (8, 8, 1):
        x = zeros()
        runs.append((solver.solve(b, x, maxiter=cap, check_every=check_every), x))
    assert runs[0][0] == runs[1][0] == runs[2][0] and runs[0][0].status == 0
    assert torch.equal(bits(runs[0][1]), bits(runs[1][1])) and torch.equal(bits(runs[0][1]), bits(runs[2][1]))
    k = runs[2][0].iterations
    x = zeros()
    before = torch.cuda.memory_allocated()
    solver.enqueue(b, x, k + 5)                                          # the five behind the stop leave x and the scalars alone
    assert torch.cuda.memory_allocated() == before
    assert solver.info() == runs[2][0]
    assert torch.equal(bits(x), bits(runs[2][1]))
    x = zeros()
    solver.enqueue(b, x, k - 1)                                          # one too few: the early exit is not what made them agree
    assert solver.info().status == KR.MAXITER and solver.info().iterations == k - 1
    assert not torch.equal(bits(x), bits(runs[2][1]))


def test_capture_behind_update(wlsqm):
    import torch
    import wlsqm.hip as whip
    name = "reaction-2D-n130"
    sy = SR.system(name)
    n, m = sy["n"], sy["m"]
    rng = np.random.default_rng(41)
    SA, SB = sy["S"], sy["S"] + 0.05 * n ** -0.5 * rng.standard_normal(sy["S"].shape)
    S = _t(SA)
    op = whip.StencilOperator(2, 2, S, _t(sy["hoods"]), _t(sy["nk"]), _t(sy["knowns"]), _t(sy["wm"]), _t(sy["rows"]))
    solver = whip.StencilSystemSolver(op, sy["coupling"], diag=sy["diag"])
    b, x0 = _t(sy["b"]), _t(rng.standard_normal((n, m)))
    x = _nan(n, m)
    iters = 2 * SR.CAPS[name]["jacobi"]                                  # a count to enqueue, not a bound

    def step():
        x.copy_(x0)
        op.update(S, check=False)
        solver.enqueue(b, x, iters)

    step()
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
    x.copy_(x0)
    assert solver.solve(b, x, maxiter=iters) == info_b and torch.equal(bits(x), bits(eager))
    solver.close(); op.close()


def test_refresh_after_a_changed_diag_tensor(wlsqm):
    import torch
    import wlsqm.hip as whip
    m = _system("random-m2")
    sy = m["sy"]
    cap = SR.CAPS["random-m2"]["jacobi"]
    diag = _t(sy["diag"])
    solver = whip.StencilSystemSolver(m["op"], sy["coupling"], diag=diag)
    zeros = lambda: torch.zeros((sy["n"], sy["m"]), dtype=torch.float64, device="cuda")
    x1 = zeros()
    first = solver.solve(m["b"], x1, maxiter=cap)
    diag.mul_(1.5)
    assert solver.refresh() is solver
    x2 = zeros()
    second = solver.solve(m["b"], x2, maxiter=cap)
    fresh = whip.StencilSystemSolver(m["op"], sy["coupling"], diag=_t(1.5 * sy["diag"]))
    x3 = zeros()
    third = fresh.solve(m["b"], x3, maxiter=cap)
    assert first.status == second.status == 0 and second == third
    assert torch.equal(bits(x2), bits(x3)) and not torch.equal(bits(x1), bits(x2))
    M = SR.dense_matrix(np.stack([m["op"].to_sparse_csr(o).to_dense().cpu().numpy() for o in range(sy["nop"])]), sy["coupling"], 1.5 * sy["diag"])
    assert np.linalg.norm(m["bflat"] - M @ x2.cpu().numpy().reshape(-1)) <= 2 * m["stop"]
    solver.close(); fresh.close()


# ---- 4. statuses, not faults --------------------------------------------------------------------------------------------------------------

def test_statuses(wlsqm):
    import torch
    import wlsqm.hip as whip
    m = _system("random-m3")
    sy, solver = m["sy"], _solver(m, "jacobi")
    n, mm = sy["n"], sy["m"]
    zeros = lambda: torch.zeros((n, mm), dtype=torch.float64, device="cuda")
    x = zeros()
    info = solver.solve(zeros(), x)                                      # b = 0 from x = 0: converged before the first iteration
    assert (info.status, info.iterations, info.residual) == (0, 0, 0.0) and torch.all(x == 0.0)
    x0 = np.random.default_rng(71).standard_normal((n, mm))
    x = _t(x0)
    info = solver.solve(m["b"], x, maxiter=0)
    assert (info.status, info.iterations) == (KR.MAXITER, 0) and _same_bits(x.cpu().numpy(), x0)
    bn = m["b"].clone()
    bn[3, 1] = float("nan")
    x = _t(x0)
    info = solver.solve(bn, x)
    assert info.status == KR.NONFINITE and info.iterations == 0 and _same_bits(x.cpu().numpy(), x0)
    x = zeros()
    info = solver.solve(m["b"], x, maxiter=2)
    xr, its_r, st_r, hist = SR.solve_ref(m["M"], m["bflat"], "jacobi", cap=2)
    assert (info.status, info.iterations) == (KR.MAXITER, 2) == (st_r, its_r) and info.residual > m["stop"]
    # a zero coupled diagonal: unknown (5, 1) has D_11 = 0 and no own entry
    st = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in sy["st"].items()}
    st["nk"][5], st["own_mask"][5] = 0, False
    op = _operator(whip, st)
    d = sy["diag"].copy()
    d[1, 1, 5] = 0.0
    zero_diag = whip.StencilSystemSolver(op, sy["coupling"], diag=_t(d))
    x = _t(x0)
    info = zero_diag.solve(m["b"], x)
    assert info.status == KR.DIAGONAL and info.iterations == 0 and _same_bits(x.cpu().numpy(), x0)
    d[1, 1, 5] = float("inf")
    inf_diag = whip.StencilSystemSolver(op, sy["coupling"], diag=_t(d))
    info = inf_diag.solve(m["b"], x)
    assert info.status == KR.DIAGONAL and _same_bits(x.cpu().numpy(), x0)
    zero_diag.close(); inf_diag.close(); op.close()


# ---- 5. no disturbance --------------------------------------------------------------------------------------------------------------------

def test_a_stencil_solver_beside_it_is_not_disturbed(wlsqm):
    import torch
    import wlsqm.hip as whip
    from wlsqm import _binding
    m = _system("random-m2")
    sy, op = m["sy"], m["op"]
    n = sy["n"]
    rows = SR.rows_of_structure(sy["st"])
    d = 1.0 + 1.5 * 0.75 * np.array([sum(abs(v[0]) for _, v in r) for r in rows])
    rng = np.random.default_rng(73)
    b1, v1 = _t(rng.standard_normal(n)), _t(rng.standard_normal(n))

    def single(solver):
        x = torch.zeros(n, dtype=torch.float64, device="cuda")
        info = solver.solve(b1, x, maxiter=100)
        after_solve = whip.last_kernel()
        prod = solver.product(v1)
        return info, x, after_solve, whip.last_kernel(), prod[0], prod[1:], solver.memory_used()

    alone = whip.StencilSolver(op, o=0, diag=_t(d), scale=-0.75)
    ref = single(alone)
    assert ref[0].status == 0 and ref[2:4] == ("krylov-update", "krylov-spmv-dot")
    assert ref[6] == _binding.lib().wlsqm_hip_krylov_workspace_bytes(n)
    system = _solver(m, "jacobi")
    cap = SR.CAPS["random-m2"]["jacobi"]
    xs = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
    info_s = system.solve(m["b"], xs, maxiter=cap)
    # interleaved: the system solver is stopped short, the single-field solver runs a whole solve, the system solver solves again
    xs2 = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
    system.enqueue(m["b"], xs2, 3)
    assert whip.last_kernel() == "krylov-update" and system.info().status == KR.MAXITER
    beside = single(alone)
    xs2.zero_()
    assert system.solve(m["b"], xs2, maxiter=cap) == info_s and torch.equal(bits(xs2), bits(xs))
    after = single(alone)
    for got in (beside, after):
        assert got[0] == ref[0] and torch.equal(bits(got[1]), bits(ref[1])) and got[2:4] == ref[2:4]
        assert torch.equal(bits(got[4]), bits(ref[4])) and got[5] == ref[5] and got[6] == ref[6]
    assert system.memory_used() == _binding.lib().wlsqm_hip_krylov_workspace_bytes(2 * n)
    alone.close()
