"""GPU tests of BiCGSTAB(2) (wlsqm.hip.StencilSolver(method="bicgstab2"), csrc/krylov.hip's krylov_l2_* kernels).

  1. solves of the systems of tests/_krylov_l2_ref.py on clouds in Morton order, with no preconditioner, Jacobi and blocks, by the criteria
     of tests/test_gpu_krylov.py against bicgstab2_ref on the operator's own values: status 0, iterations within the cap that
     tests/test_krylov_l2_host.py ties to the reference's count, the true residual within max(rtol ||b||, atol) + 8 gap, the error
     against the direct solve within kappa_2(M) times the relative residual;
  2. the headline: I - h^2 Lap_h in 3D at n = 1000 and n = 2000 with blocks of 16, where BiCGSTAB with the same blocks breaks down;
  3. a transposed solve, and dL/db through differentiable_stencil_solve;
  4. every size at which the kernels take another path; 5. determinism, capture, refresh=False; 6. statuses, never a fault;
  7. the default method is untouched; 8. refusals.
"""
import numpy as np
import pytest

import _krylov_block_ref as KB
import _krylov_l2_ref as L2
import _krylov_ref as KR
import _stencil_ref as R
from _device_helpers import bits, dev as _t, nan as _nan, same_bits as _same_bits, wlsqm  # noqa: F401 (fixture)
from test_gpu_krylov import _build

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 300, 65537)


def _zeros(n):
    import torch
    return torch.zeros(n, dtype=torch.float64, device="cuda")


def _preconditioner(whip, pc):
    return whip.BlockJacobi(pc) if isinstance(pc, int) else pc


_made = {}


def _system(name):
    """The system `name` on a cloud in Morton order, on the device, and what the tests share about it, computed once and left unchanged."""
    if name not in _made:
        import wlsqm.hip as whip
        sy = L2.system(name)
        op, args = _build(whip, sy)
        M = KR.dense_of(sy, op.to_sparse_csr(0).to_dense().cpu().numpy())
        _made[name] = dict(sy=sy, op=op, args=args, M=M, b=_t(sy["b"]), stop=KR.RTOL * np.linalg.norm(sy["b"]), solvers={})
    return _made[name]


def _solver(m, pc, method="bicgstab2"):
    import wlsqm.hip as whip
    if (pc, method) not in m["solvers"]:
        m["solvers"][pc, method] = whip.StencilSolver(m["op"], preconditioner=_preconditioner(whip, pc), method=method, **m["args"])
    return m["solvers"][pc, method]


def _held_to_the_reference(M, b, x, info, pc, cap, what, error=True):
    """tests/test_gpu_krylov.py's criteria of a solve, against bicgstab2_ref with the same preconditioner on the same matrix."""
    xr, its_r, st_r, hist = L2.bicgstab2_ref(M, b, np.zeros(len(b)), L2.preconditioner(M, pc), KR.RTOL, 0.0, cap)
    assert st_r == KR.CONVERGED, (what, st_r, its_r)
    stop = KR.RTOL * np.linalg.norm(b)
    gap = abs(np.linalg.norm(b - M @ xr) - hist[-1])
    true = np.linalg.norm(b - M @ x)
    print("%s: iterations %d (reference %d, cap %d), recursive %.3e true %.3e stop %.3e gap %.3e"
          % (what, info.iterations, its_r, cap, info.residual, true, stop, gap))
    assert info.status == KR.CONVERGED, (what, info)
    assert 0 < info.iterations <= cap and info.iterations % 2 == 0, (what, info)
    assert info.residual <= stop
    assert true <= stop + 8 * gap, (what, true, stop, gap)
    if error:
        xstar, kappa = np.linalg.solve(M, b), np.linalg.cond(M)
        err = np.linalg.norm(x - xstar) / np.linalg.norm(xstar)
        print("%s: error %.3e bound %.3e" % (what, err, kappa * true / np.linalg.norm(b)))
        assert err <= kappa * true / np.linalg.norm(b) * (1 + 1e-6), (what, err)


# ---- 1. solves ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,pc", L2.GPU_CASES)
def test_solve(wlsqm, name, pc):
    import wlsqm.hip as whip
    m = _system(name)
    n, cap = m["sy"]["n"], L2.CAPS[name][pc]
    x = _zeros(n)
    info = _solver(m, pc).solve(m["b"], x, rtol=KR.RTOL, maxiter=cap)
    assert whip.last_kernel() == ("krylov-l2-update-block" if isinstance(pc, int) else "krylov-l2-update")
    _held_to_the_reference(m["M"], m["sy"]["b"], x.cpu().numpy(), info, pc, cap, "%s %s" % (name, pc))


# ---- 2. the headline --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(L2.HEADLINE))
def test_large_step_in_3d_where_bicgstab_breaks_down(wlsqm, name):
    m = _system(name)
    n, cap = m["sy"]["n"], L2.HEADLINE[name]
    x = _zeros(n)
    info = _solver(m, 16).solve(m["b"], x, rtol=KR.RTOL, maxiter=cap, check_every=64)
    y = _zeros(n)
    other = _solver(m, 16, "bicgstab").solve(m["b"], y, rtol=KR.RTOL, maxiter=4 * cap, check_every=64)
    print("%s, blocks of 16: bicgstab2 %s; bicgstab %s, true residual %.3e" % (name, info, other, np.linalg.norm(m["sy"]["b"] - m["M"] @ y.cpu().numpy())))
    # the error criterion wants kappa_2 of a 2000 x 2000 matrix: the residual criterion alone at that size
    _held_to_the_reference(m["M"], m["sy"]["b"], x.cpu().numpy(), info, 16, cap, name, error=n <= 1000)


# ---- 3. transposed solves and autograd ------------------------------------------------------------------------------------------------------

def test_transposed_solve_and_autograd(wlsqm):
    import wlsqm.hip as whip
    name, pc, cap = L2.TRANSPOSED
    m = _system(name)
    n = m["sy"]["n"]
    solver = whip.StencilSolver(m["op"], preconditioner=whip.BlockJacobi(pc), method="bicgstab2", **m["args"])
    x = _zeros(n)
    info = solver.solve(m["b"], x, rtol=KR.RTOL, maxiter=cap, transpose=True)
    MT = np.ascontiguousarray(m["M"].T)
    _held_to_the_reference(MT, m["sy"]["b"], x.cpu().numpy(), info, pc, cap, "transposed")      # the blocks of M^T: the transposed blocks
    # dL/db of L = (w, x): the backward pass is solve(transpose=True) on the solver that it is given
    w = _t(np.random.default_rng(83).standard_normal(n))
    grads = []
    default = whip.StencilSolver(m["op"], **m["args"])
    for s in (solver, default):
        b = m["b"].clone().requires_grad_(True)
        xs = whip.differentiable_stencil_solve(s, b, rtol=KR.RTOL, maxiter=1000)
        (xs * w).sum().backward()
        assert whip.last_kernel().startswith("krylov-l2-update" if s is solver else "krylov-update")
        grads.append(b.grad.cpu().numpy())
    diff, size, kappa = np.linalg.norm(grads[0] - grads[1]), np.linalg.norm(grads[1]), np.linalg.cond(m["M"])
    print("dL/db: bicgstab2 against the default solver %.3e of %.3e, bound %.3e" % (diff, size, kappa * KR.RTOL * size))
    assert diff <= kappa * KR.RTOL * size
    solver.close(); default.close()


# ---- 4. sizes -------------------------------------------------------------------------------------------------------------------------------

class _Sparse:
    """M = diag(d) + c A of a large structure as what bicgstab2_ref needs of a matrix: M @ v, on the host, from the operator's CSR."""

    def __init__(self, row, col, val, d, c):
        self.row, self.col, self.val, self.d, self.c = row, col, val, d, c

    def __matmul__(self, v):
        return self.d * v + self.c * np.bincount(self.row, weights=self.val * v[self.col], minlength=len(v))


@pytest.mark.parametrize("n", SIZES)
def test_sizes(wlsqm, n):
    """Empty rows, an empty slice (rows 64 .. 127 from 130 rows on), more than one workgroup, and the reduce's loop from 257 workgroups
    on.  After two cycles at rtol = 0 the workspace's r is b - M x within the bound that tests/test_krylov_host.py holds the reference's
    own gap to: per iteration 10 gamma_{L+4} (|M| |x| + |b|), L the longest row."""
    import wlsqm.hip as whip
    st = KR.square_structure(n, 9, seed=31)
    op = whip.StencilOperator.from_coefficients(_t(st["hoods"]), _t(st["nk"]), _t(st["slots"]), n, own=_t(st["own"]), own_mask=_t(st["own_mask"]))
    csr = op.to_sparse_csr(0).cpu()
    col, val = csr.col_indices().numpy(), csr.values().numpy()
    lens = np.diff(csr.crow_indices().numpy())
    row = np.repeat(np.arange(n), lens)
    if n >= 300:
        assert lens.min() == 0 and np.all(lens[64:128] == 0)
    c = -0.75
    d = 1.0 + 1.5 * abs(c) * np.bincount(row, weights=np.abs(val), minlength=n)
    M, absM = _Sparse(row, col, val, d, c), _Sparse(row, col, np.abs(val), d, abs(c))
    b = np.random.default_rng([97, n]).standard_normal(n)
    room = lambda its, x: its * 10 * R.gamma(int(lens.max()) + 5) * (np.linalg.norm(absM @ np.abs(x)) + np.linalg.norm(b))
    for pc in (None, "jacobi", 16):
        solver = whip.StencilSolver(op, diag=_t(d), scale=c, preconditioner=_preconditioner(whip, pc), method="bicgstab2")
        assert solver.memory_used() - (0 if pc != 16 else 8 * (64 * 16 * ((n + 63) // 64) + (n + 255) // 256)) \
            == wlsqm._binding.lib().wlsqm_hip_krylov_l2_workspace_bytes(n) == 8 * (16 + 5 * ((n + 255) // 256) + 10 * n)
        dinv = 1.0 / (d + c * np.bincount(row[row == col], weights=val[row == col], minlength=n))      # the diagonal of M
        if pc == 16:
            W = solver.preconditioner_blocks().cpu().numpy()
            pre = lambda z: KB.apply_blocks(W, z)
        else:
            pre = dinv if pc == "jacobi" else None
        x = _zeros(n)
        info = solver.solve(_t(b), x, rtol=KR.RTOL, maxiter=100)
        xr, its_r, st_r, hist = L2.bicgstab2_ref(M, b, np.zeros(n), pre, KR.RTOL, 0.0, 100)
        xh = x.cpu().numpy()
        stop, true, gap = KR.RTOL * np.linalg.norm(b), np.linalg.norm(b - M @ xh), abs(np.linalg.norm(b - M @ xr) - hist[-1])
        print("n %d %s: %s (reference %d iterations), true %.3e stop %.3e gap %.3e" % (n, pc, info, its_r, true, stop, gap))
        assert st_r == KR.CONVERGED and info.status == KR.CONVERGED and 0 < info.iterations <= 2 * its_r
        assert np.isfinite(xh).all() and info.residual <= stop and true <= stop + 8 * gap
        # two cycles without a stop, then r of the workspace (its first vector, behind the scalars and the 5 planes of partials)
        x = _zeros(n)
        solver.enqueue(_t(b), x, 4, rtol=0.0)
        info = solver.info()
        xr, its_r, st_r, hist = L2.bicgstab2_ref(M, b, np.zeros(n), pre, 0.0, 0.0, 4)
        if n > 1:
            assert (info.status, info.iterations) == (st_r, its_r) == (KR.MAXITER, 4), (n, pc, info, st_r, its_r)
        if info.status in (KR.MAXITER, KR.CONVERGED):                     # one row: r may vanish, and the second cycle break down
            at = 16 + 5 * ((n + 255) // 256)
            r, xh = solver._ws[at:at + n].cpu().numpy(), x.cpu().numpy()
            drift, drift_r = np.linalg.norm(r - (b - M @ xh)), abs(np.linalg.norm(b - M @ xr) - hist[-1])
            print("n %d %s: after two cycles |r - (b - M x)| %.3e, the reference's gap %.3e, room %.3e" % (n, pc, drift, drift_r, room(4, xh)))
            assert drift_r <= room(4, xr) and drift <= room(4, xh)
        solver.close()
    op.close()


# ---- 5. determinism, capture, refresh=False ---------------------------------------------------------------------------------------------------

def test_same_bits_twice_and_behind_the_stop(wlsqm):
    import torch
    name = "2D-tau1-n130"
    m = _system(name)
    for pc in (16, "jacobi"):
        solver, b, n, cap = _solver(m, pc), m["b"], m["sy"]["n"], L2.CAPS[name][pc]
        runs = []
        for check_every in (8, 1, 1):
            x = _zeros(n)
            runs.append((solver.solve(b, x, maxiter=cap, check_every=check_every), x))
        assert runs[0][0] == runs[1][0] == runs[2][0] and runs[0][0].status == 0
        assert torch.equal(bits(runs[0][1]), bits(runs[1][1])) and torch.equal(bits(runs[1][1]), bits(runs[2][1]))
        k = runs[1][0].iterations
        x = _zeros(n)
        before = torch.cuda.memory_allocated()
        solver.enqueue(b, x, k + 6)
        assert torch.cuda.memory_allocated() == before
        assert solver.info() == runs[1][0] and torch.equal(bits(x), bits(runs[1][1]))
        x = _zeros(n)
        solver.enqueue(b, x, k - 2)                                      # one cycle less
        assert solver.info().status == KR.MAXITER and solver.info().iterations == k - 2
        assert not torch.equal(bits(x), bits(runs[1][1]))
        x = _zeros(n)
        solver.enqueue(b, x, k - 3)                                      # ceil((k - 3) / 2) cycles: an odd limit is passed by one
        assert solver.info().status == KR.MAXITER and solver.info().iterations == k - 2


def _moving(whip, refresh):
    name = "2D-tau0.25-n130"
    sy = KB.morton_system(name)
    n = sy["n"]
    rng = np.random.default_rng(41)
    SA, SB = sy["S"], sy["S"] + 0.05 * n ** -0.5 * rng.standard_normal(sy["S"].shape)
    S = _t(SA)
    op = whip.StencilOperator(2, 2, S, _t(sy["hoods"]), _t(sy["nk"]), _t(sy["knowns"]), _t(sy["wm"]), _t(sy["rows"]))
    solver = whip.StencilSolver(op, diag=sy["diag"], scale=sy["scale"], preconditioner=whip.BlockJacobi(16, refresh=refresh), method="bicgstab2")
    return sy, n, SA, SB, S, op, solver


def test_capture_behind_update(wlsqm):
    import torch
    import wlsqm.hip as whip
    sy, n, SA, SB, S, op, solver = _moving(whip, True)
    b, x0 = _t(sy["b"]), _t(KR.guess(n))
    x = _nan(n)
    iters = 40                                                           # a count to enqueue, not a bound: the solves stop long before

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
    solver.close(); op.close()


def test_refresh_false_keeps_the_blocks_until_refresh(wlsqm):
    import torch
    import wlsqm.hip as whip
    sy, n, SA, SB, S, op, solver = _moving(whip, False)
    b, x0 = _t(sy["b"]), _t(KR.guess(n))
    x = _nan(n)

    def step():
        x.copy_(x0)
        op.update(S, check=False)
        solver.enqueue(b, x, 40)

    step()                                                               # the first start factors
    P_a, info_a = solver.preconditioner_blocks(), solver.info()
    S.copy_(_t(SB))
    step()
    stale, info_stale = x.clone(), solver.info()
    assert info_a.status == info_stale.status == 0                       # the old P on the moved operator still converges
    assert torch.equal(bits(solver.preconditioner_blocks()), bits(P_a))
    solver.refresh()
    P_b = solver.preconditioner_blocks()
    assert not torch.equal(bits(P_b), bits(P_a))
    step()
    assert solver.info().status == 0 and torch.equal(bits(solver.preconditioner_blocks()), bits(P_b))
    # the refreshed P is what a refresh=True solver computes on the moved operator, and so is the solve
    fresh = whip.StencilSolver(op, diag=sy["diag"], scale=sy["scale"], preconditioner=whip.BlockJacobi(16), method="bicgstab2")
    y = x0.clone()
    fresh.enqueue(b, y, 40)
    assert fresh.info() == solver.info() and torch.equal(bits(y), bits(x))
    assert not torch.equal(bits(stale), bits(x))
    assert np.linalg.norm((stale - x).cpu().numpy()) <= 1e-8 * np.linalg.norm(x.cpu().numpy())      # two routes to one solution
    fresh.close(); solver.close(); op.close()


# ---- 6. statuses, never a fault -----------------------------------------------------------------------------------------------------------

def test_statuses_without_a_fault(wlsqm):
    import torch
    import wlsqm.hip as whip
    m = _system("random-n130")
    n, b = m["sy"]["n"], m["b"]
    x0 = KR.guess(n)
    for pc in (None, "jacobi", 16):
        solver = _solver(m, pc)
        x = _zeros(n)
        info = solver.solve(_zeros(n), x)
        assert (info.status, info.iterations, info.residual) == (KR.CONVERGED, 0, 0.0) and not x.any()
        x = _t(x0)
        info = solver.solve(b, x, maxiter=0)
        assert (info.status, info.iterations) == (KR.MAXITER, 0) and _same_bits(x.cpu().numpy(), x0)
        bn = b.clone()
        bn[3] = float("nan")
        x = _t(x0)
        info = solver.solve(bn, x)
        assert (info.status, info.iterations) == (KR.NONFINITE, 0) and _same_bits(x.cpu().numpy(), x0)
        solver.enqueue(bn, x, 6)                                          # what is enqueued behind the stop leaves x alone
        assert solver.info().status == KR.NONFINITE and _same_bits(x.cpu().numpy(), x0)
        x = _zeros(n)
        assert solver.solve(b, x, maxiter=L2.CAPS["random-n130"][pc]).status == KR.CONVERGED        # the solver is none the worse
    # an unusable block: [[1, 1], [1, 1]] inside every leading block, on a regular matrix
    st = KB.singular_block_structure()
    ns = st["npoints"]
    op = whip.StencilOperator.from_coefficients(_t(st["hoods"]), _t(st["nk"]), _t(st["slots"]), ns, own=_t(st["own"]), own_mask=_t(st["own_mask"]))
    bs, xs0 = _t(np.random.default_rng(89).standard_normal(ns)), KR.guess(ns)
    for nb in KB.BLOCKS:
        solver = whip.StencilSolver(op, diag=KB.SINGULAR_DIAG, scale=1.0, preconditioner=whip.BlockJacobi(nb), method="bicgstab2")
        x = _t(xs0)
        info = solver.solve(bs, x)
        assert info.status == KR.DIAGONAL and info.iterations == 0 and _same_bits(x.cpu().numpy(), xs0), (nb, info)
        solver.close()
    jacobi = whip.StencilSolver(op, diag=KB.SINGULAR_DIAG, scale=1.0, method="bicgstab2")
    x = _zeros(ns)
    assert jacobi.solve(bs, x, maxiter=500).status == KR.CONVERGED       # the matrix is regular, and its diagonal is usable
    jacobi.close(); op.close()
    # a zero diagonal under Jacobi: an empty slice with diag = 0
    st = KR.square_structure(130, 9, seed=31)
    op = whip.StencilOperator.from_coefficients(_t(st["hoods"]), _t(st["nk"]), _t(st["slots"]), 130, own=_t(st["own"]), own_mask=_t(st["own_mask"]))
    assert (np.asarray(st["nk"][64:128]) == 0).all()
    solver = whip.StencilSolver(op, diag=0.0, scale=1.0, method="bicgstab2")
    x = _t(x0)
    info = solver.solve(b, x)
    assert info.status == KR.DIAGONAL and info.iterations == 0 and _same_bits(x.cpu().numpy(), x0)
    solver.close(); op.close()
    # the exchange matrix [[0, 1], [1, 0]] with b = e_1: u1 = M r = e_2, so (rt, u1) = 0
    hoods = np.array([[1], [0]], np.int32)
    op = whip.StencilOperator.from_coefficients(_t(hoods), _t(np.ones(2, np.int32)), _t(np.ones((1, 2, 1))), 2)
    assert np.array_equal(op.to_sparse_csr(0).to_dense().cpu().numpy(), [[0.0, 1.0], [1.0, 0.0]])
    solver = whip.StencilSolver(op, diag=0.0, scale=1.0, preconditioner=None, method="bicgstab2")
    x = _zeros(2)
    info = solver.solve(_t(np.array([1.0, 0.0])), x)
    assert (info.status, info.iterations) == (KR.BREAKDOWN, 0) and not x.any()
    assert L2.bicgstab2_ref(np.array([[0.0, 1.0], [1.0, 0.0]]), np.array([1.0, 0.0]), np.zeros(2), None, 1e-10, 0.0, 10)[1:3] == (0, KR.BREAKDOWN)
    solver.close(); op.close()


# ---- 7. the default method is untouched -------------------------------------------------------------------------------------------------------

def test_the_default_method_is_unchanged(wlsqm):
    import torch
    import wlsqm.hip as whip
    m = _system("2D-tau0.25-n130")
    n = m["sy"]["n"]
    for pc, family in (("jacobi", "krylov-update"), (None, "krylov-update"), (16, "krylov-update-block")):
        got = []
        for kw in ({}, {"method": "bicgstab"}):
            solver = whip.StencilSolver(m["op"], preconditioner=_preconditioner(whip, pc), **kw, **m["args"])
            assert solver.method == "bicgstab"
            assert solver.memory_used() - (0 if pc != 16 else wlsqm._binding.lib().wlsqm_hip_krylov_block_bytes(n, 16)) \
                == wlsqm._binding.lib().wlsqm_hip_krylov_workspace_bytes(n)
            x = _zeros(n)
            info = solver.solve(m["b"], x, rtol=KR.RTOL, maxiter=100)
            assert whip.last_kernel() == family
            solver.enqueue(m["b"], x, 0)
            assert whip.last_kernel() == "krylov-reduce"
            got.append((info, x, solver._ws[:16].clone()))
            solver.close()
        assert got[0][0] == got[1][0] and got[0][0].status == 0
        assert torch.equal(bits(got[0][1]), bits(got[1][1]))


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------

def test_refusals(wlsqm):
    import wlsqm.hip as whip
    m = _system("2D-tau0.25-n130")
    with pytest.raises(ValueError, match="method must be 'bicgstab' or 'bicgstab2'; got 'gmres'"):
        whip.StencilSolver(m["op"], method="gmres", **m["args"])
    with pytest.raises(ValueError, match="method 'bicgstab2' solves one right-hand side at a time: nfields must be 1; got 2"):
        whip.StencilSolver(m["op"], method="bicgstab2", nfields=2, **m["args"])
    solver = _solver(m, "jacobi")
    with pytest.raises(ValueError, match="belongs to a BlockJacobi preconditioner"):
        solver.refresh()
    with pytest.raises(ValueError, match="the number of iterations must be"):
        solver.enqueue(m["b"], _zeros(m["sy"]["n"]), -1)
