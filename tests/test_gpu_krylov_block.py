"""GPU tests of the block-Jacobi preconditioner (wlsqm.hip.BlockJacobi, csrc/krylov.hip's krylov_blocks_kernel, krylov_update_block_kernel
and krylov_precondition_kernel).

  1. precondition(v) against the block solve in mpmath, per block within f * nb eps kappa_inf(B) |z_ref|_inf with f = 4 times what the
     numpy statement of the elimination showed on the host (tests/test_krylov_block_host.py; the margin is for fma and the order in
     which the lanes take the pivot row), on random square structures of every size at which the kernels take another path — one row, a
     last block of 1 / 15 / 16 rows, one slice less one, one slice, two slices, an empty slice, more than one workgroup — and on a fit;
     preconditioner_blocks() holds the identity in the padding of the last block;
  2. solves of the systems of tests/_krylov_block_ref.py on clouds in Morton order by the criteria of tests/test_gpu_krylov.py, against the
     block-preconditioned reference on the operator's own values;
  3. what the feature is for: at most half the iterations of Jacobi on I - h^2 Lap_h;
  4. transposed solves and autograd through a block solver; 5. determinism, capture, refresh=False; 6. status 4, never a fault;
  7. refusals that need a device.
"""
import numpy as np
import pytest

import _krylov_block_ref as KB
import _krylov_ref as KR
from _device_helpers import bits, dev as _t, nan as _nan, same_bits as _same_bits, wlsqm  # noqa: F401 (fixture)
from test_gpu_krylov import _build

pytestmark = pytest.mark.gpu

SIZES = (1, 15, 16, 17, 63, 64, 65, 130, 300)
F = 4.0 * KB.STATEMENT_RATIO


def _zeros(n):
    import torch
    return torch.zeros(n, dtype=torch.float64, device="cuda")


_made = {}


def _system(name):
    """The system `name` on a cloud in Morton order, on the device, and what the tests share about it, computed once and left unchanged."""
    if name not in _made:
        import wlsqm.hip as whip
        sy = KB.morton_system(name)
        op, args = _build(whip, sy)
        M = KR.dense_of(sy, op.to_sparse_csr(0).to_dense().cpu().numpy())
        _made[name] = dict(sy=sy, op=op, args=args, M=M, b=_t(sy["b"]), xstar=np.linalg.solve(M, sy["b"]),
                           stop=KR.RTOL * np.linalg.norm(sy["b"]), kappa=np.linalg.cond(M), solvers={})
    return _made[name]


def _solver(m, nb):
    import wlsqm.hip as whip
    if nb not in m["solvers"]:
        m["solvers"][nb] = whip.StencilSolver(m["op"], preconditioner=whip.BlockJacobi(nb), **m["args"])
    return m["solvers"][nb]


def _held_to_the_reference(M, b, x, info, pre, cap, what, x0=None):
    """tests/test_gpu_krylov.py's criteria of a solve, against the reference run with the preconditioner `pre` on the same matrix."""
    n = len(b)
    xr, its_r, st_r, hist = KB.bicgstab_block_ref(M, b, np.zeros(n) if x0 is None else x0, pre, KR.RTOL, 0.0, cap)
    assert st_r == KR.CONVERGED, (what, st_r, its_r)
    xstar = np.linalg.solve(M, b)
    stop, kappa = KR.RTOL * np.linalg.norm(b), np.linalg.cond(M)
    gap = abs(np.linalg.norm(b - M @ xr) - hist[-1])
    true = np.linalg.norm(b - M @ x)
    err = np.linalg.norm(x - xstar) / np.linalg.norm(xstar)
    print("%s: iterations %d (reference %d, cap %d), recursive %.3e true %.3e stop %.3e gap %.3e, error %.3e bound %.3e"
          % (what, info.iterations, its_r, cap, info.residual, true, stop, gap, err, kappa * true / np.linalg.norm(b)))
    assert info.status == KR.CONVERGED, (what, info)
    assert 0 < info.iterations <= cap, (what, info)
    assert info.residual <= stop
    assert true <= stop + 8 * gap, (what, true, stop, gap)
    assert err <= kappa * true / np.linalg.norm(b) * (1 + 1e-6), (what, err)


# ---- 1. the inverses ------------------------------------------------------------------------------------------------------------------

def _structure(whip, n, seed=31):
    st = KR.square_structure(n, 9, seed=seed)
    op = whip.StencilOperator.from_coefficients(_t(st["hoods"]), _t(st["nk"]), _t(st["slots"]), n, own=_t(st["own"]), own_mask=_t(st["own_mask"]))
    return st, op


@pytest.mark.parametrize("n", SIZES)
def test_precondition_against_the_mpmath_block_solve(wlsqm, n):
    import torch
    import wlsqm.hip as whip
    st, op = _structure(whip, n)
    rng = np.random.default_rng([71, n])
    d, c = rng.standard_normal(n), -0.75
    v = rng.standard_normal(n) * 10.0 ** rng.integers(-2, 3, n)
    M = KR.dense_of(dict(kind="random", st=st, diag=d, scale=c, n=n))
    for nb in KB.BLOCKS:
        solver = whip.StencilSolver(op, diag=_t(d), scale=c, preconditioner=whip.BlockJacobi(nb))
        assert solver.memory_used() == wlsqm._binding.lib().wlsqm_hip_krylov_workspace_bytes(n) + 8 * (64 * nb * ((n + 63) // 64) + (n + 255) // 256)
        out = _nan(n)
        z = solver.precondition(_t(v), out=out)
        assert z is out and whip.last_kernel() == "krylov-precondition"
        blocks = KB.blocks_of(M, nb)
        ratio = KB.worst_ratio(blocks, z.cpu().numpy(), KB.mp_block_solve(blocks, v), nb)
        zt = solver.precondition(_t(v), transpose=True).cpu().numpy()
        blocks_t = np.ascontiguousarray(blocks.transpose(0, 2, 1))
        ratio_t = KB.worst_ratio(blocks_t, zt, KB.mp_block_solve(blocks_t, v), nb)
        print("n %d block %d: worst ratio %.3f, transposed %.3f (bound %.3f)" % (n, nb, ratio, ratio_t, F))
        assert np.isfinite(z.cpu().numpy()).all() and ratio <= F and ratio_t <= F
        W = solver.preconditioner_blocks()
        nblocks = (n + nb - 1) // nb
        assert tuple(W.shape) == (nblocks, nb, nb) and whip.last_kernel() == "krylov-blocks"
        W = W.cpu().numpy()
        last = n - (nblocks - 1) * nb
        pad = W[-1].copy()
        pad[:last, :last] = np.eye(nb)[:last, :last]
        assert np.array_equal(pad, np.eye(nb))                            # the identity in the padding, exact zeros beside it
        # precondition is these blocks applied: nb terms with fma against numpy's sum of the same terms
        za = KB.apply_blocks(W, v)
        assert np.all(np.abs(za - z.cpu().numpy()) <= 2 * nb * KB.EPS * KB.apply_blocks(np.abs(W), np.abs(v)))
        again = solver.precondition(_t(v))
        assert torch.equal(bits(again), bits(z))
        solver.close()
    op.close()


def test_precondition_on_a_fitted_operator(wlsqm):
    m = _system("2D-tau1-n130")
    n = m["sy"]["n"]
    v = np.random.default_rng(73).standard_normal(n)
    for nb in KB.BLOCKS:
        solver = _solver(m, nb)
        blocks = KB.blocks_of(m["M"], nb)
        z = solver.precondition(_t(v)).cpu().numpy()
        ratio = KB.worst_ratio(blocks, z, KB.mp_block_solve(blocks, v), nb)
        print("fit, block %d: worst ratio %.3f (bound %.3f), worst kappa_inf %.3g" % (nb, ratio, F, max(KB.kappa_inf(B) for B in blocks)))
        assert ratio <= F


# ---- 2. solves ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,nb", [(name, nb) for name, caps in KB.GPU_CAPS.items() for nb in caps])
def test_solve(wlsqm, name, nb):
    import wlsqm.hip as whip
    m = _system(name)
    n, cap = m["sy"]["n"], KB.CAPS[name][nb]
    x = _zeros(n)
    info = _solver(m, nb).solve(m["b"], x, rtol=KR.RTOL, maxiter=cap)
    assert whip.last_kernel() == "krylov-update-block"
    _held_to_the_reference(m["M"], m["sy"]["b"], x.cpu().numpy(), info, KB.block_preconditioner(m["M"], nb), cap, "%s block %d" % (name, nb))


# ---- 3. what it is for ------------------------------------------------------------------------------------------------------------------

def test_half_the_iterations_of_jacobi(wlsqm):
    import wlsqm.hip as whip
    m = _system("2D-tau1-n130")
    n = m["sy"]["n"]
    jacobi = whip.StencilSolver(m["op"], **m["args"])
    xj, xb = _zeros(n), _zeros(n)
    ij = jacobi.solve(m["b"], xj, rtol=KR.RTOL, maxiter=1000)
    ib = _solver(m, 16).solve(m["b"], xb, rtol=KR.RTOL, maxiter=1000)
    print("I - h^2 Lap_h, n = 130: Jacobi %d iterations, block 16 %d" % (ij.iterations, ib.iterations))
    assert ij.status == ib.status == 0 and 0 < 2 * ib.iterations <= ij.iterations
    jacobi.close()


# ---- 4. transposed solves ---------------------------------------------------------------------------------------------------------------

def test_transposed_solve_and_autograd(wlsqm):
    import torch
    import wlsqm.hip as whip
    name, nb, cap = KB.TRANSPOSED
    m = _system(name)
    n = m["sy"]["n"]
    solver = whip.StencilSolver(m["op"], preconditioner=whip.BlockJacobi(nb), **m["args"])
    x = _zeros(n)
    before = solver.memory_used()
    info = solver.solve(m["b"], x, rtol=KR.RTOL, maxiter=cap, transpose=True)
    assert solver.memory_used() == 2 * before - wlsqm._binding.lib().wlsqm_hip_krylov_workspace_bytes(n)     # the transposed plane
    MT = np.ascontiguousarray(m["M"].T)
    # the blocks of M^T are the transposed blocks of M
    _held_to_the_reference(MT, m["sy"]["b"], x.cpu().numpy(), info, KB.block_preconditioner(MT, nb), cap, "transposed")
    inv, inv_t = KB.block_inverses(m["M"], nb), solver.preconditioner_blocks().cpu().numpy()
    v = np.random.default_rng(79).standard_normal(n)
    zt = solver.precondition(_t(v), transpose=True).cpu().numpy()
    assert np.allclose(zt, KB.apply_blocks(inv, v, transpose=True), rtol=1e-9, atol=1e-9 * np.abs(zt).max()) and inv_t.shape == inv.shape
    # dL/db of L = (w, x) through the two preconditioners
    w = _t(np.random.default_rng(83).standard_normal(n))
    grads = []
    jacobi = whip.StencilSolver(m["op"], **m["args"])
    for s in (solver, jacobi):
        b = m["b"].clone().requires_grad_(True)
        xs = whip.differentiable_stencil_solve(s, b, rtol=KR.RTOL, maxiter=1000)
        (xs * w).sum().backward()
        grads.append(b.grad.cpu().numpy())
    diff, size = np.linalg.norm(grads[0] - grads[1]), np.linalg.norm(grads[1])
    print("dL/db: block against Jacobi %.3e of %.3e, bound %.3e" % (diff, size, m["kappa"] * KR.RTOL * size))
    assert diff <= m["kappa"] * KR.RTOL * size
    solver.close(); jacobi.close()


# ---- 5. determinism, capture, refresh=False -------------------------------------------------------------------------------------------------

def test_same_bits_twice_and_behind_the_stop(wlsqm):
    import torch
    name, nb = "2D-dirichlet-n130", 16
    m = _system(name)
    solver, b, n, cap = _solver(m, nb), m["b"], m["sy"]["n"], KB.CAPS[name][nb]
    runs = []
    for check_every in (8, 1, 1):
        x = _zeros(n)
        runs.append((solver.solve(b, x, maxiter=cap, check_every=check_every), x))
    assert runs[0][0] == runs[1][0] == runs[2][0] and runs[0][0].status == 0
    assert torch.equal(bits(runs[0][1]), bits(runs[1][1])) and torch.equal(bits(runs[1][1]), bits(runs[2][1]))
    k = runs[1][0].iterations
    x = _zeros(n)
    before = torch.cuda.memory_allocated()
    solver.enqueue(b, x, k + 5)
    assert torch.cuda.memory_allocated() == before
    assert solver.info() == runs[1][0] and torch.equal(bits(x), bits(runs[1][1]))
    x = _zeros(n)
    solver.enqueue(b, x, k - 1)
    assert solver.info().status == KR.MAXITER and solver.info().iterations == k - 1
    assert not torch.equal(bits(x), bits(runs[1][1]))


def _moving(whip, refresh):
    name = "2D-tau0.25-n130"
    sy = KB.morton_system(name)
    n = sy["n"]
    rng = np.random.default_rng(41)
    SA, SB = sy["S"], sy["S"] + 0.05 * n ** -0.5 * rng.standard_normal(sy["S"].shape)
    S = _t(SA)
    op = whip.StencilOperator(2, 2, S, _t(sy["hoods"]), _t(sy["nk"]), _t(sy["knowns"]), _t(sy["wm"]), _t(sy["rows"]))
    solver = whip.StencilSolver(op, diag=sy["diag"], scale=sy["scale"], preconditioner=whip.BlockJacobi(16, refresh=refresh))
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
    # a transposed use inside a capture without prepare_transpose is refused; with it, it is captured
    refused = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="the stream is capturing: call prepare_transpose before the capture"):
        with torch.cuda.graph(refused, stream=torch.cuda.Stream()):
            solver.enqueue(b, x, 3, transpose=True)
    torch.cuda.synchronize()
    assert solver.prepare_transpose() is True and solver.prepare_transpose() is False
    x.copy_(x0)
    solver.enqueue(b, x, iters, transpose=True)
    eager_t, info_t = x.clone(), solver.info()
    taken = torch.cuda.CUDAGraph()
    with torch.cuda.graph(taken, stream=torch.cuda.Stream()):
        x.copy_(x0)
        solver.enqueue(b, x, iters, transpose=True)
    torch.cuda.synchronize()
    x.fill_(float("nan"))
    taken.replay()
    torch.cuda.synchronize()
    assert info_t.status == 0 and torch.equal(bits(x), bits(eager_t)) and solver.info() == info_t
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
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        step()
    torch.cuda.synchronize()
    S.copy_(_t(SB))
    graph.replay()
    torch.cuda.synchronize()
    stale, info_stale = x.clone(), solver.info()
    assert info_a.status == info_stale.status == 0                       # the old P on the moved operator still converges
    assert torch.equal(bits(solver.preconditioner_blocks()), bits(P_a))
    solver.refresh()
    P_b = solver.preconditioner_blocks()
    assert not torch.equal(bits(P_b), bits(P_a))
    graph.replay()
    torch.cuda.synchronize()
    assert solver.info().status == 0 and torch.equal(bits(solver.preconditioner_blocks()), bits(P_b))
    # the refreshed P is what a refresh=True solver computes on the moved operator, and so is the solve
    fresh = whip.StencilSolver(op, diag=sy["diag"], scale=sy["scale"], preconditioner=whip.BlockJacobi(16))
    assert torch.equal(bits(fresh.preconditioner_blocks()), bits(P_b))
    y = x0.clone()
    fresh.enqueue(b, y, 40)
    assert fresh.info() == solver.info() and torch.equal(bits(y), bits(x))
    assert np.linalg.norm((stale - x).cpu().numpy()) <= 1e-8 * np.linalg.norm(x.cpu().numpy())      # two routes to one solution
    fresh.close(); solver.close(); op.close()


# ---- 6. status 4, not a fault -------------------------------------------------------------------------------------------------------------

def test_status_4_and_no_fault(wlsqm):
    import wlsqm.hip as whip
    st = KB.singular_block_structure()
    n = st["npoints"]
    op = whip.StencilOperator.from_coefficients(_t(st["hoods"]), _t(st["nk"]), _t(st["slots"]), n, own=_t(st["own"]), own_mask=_t(st["own_mask"]))
    b, x0 = _t(np.random.default_rng(89).standard_normal(n)), KR.guess(n)
    jacobi = whip.StencilSolver(op, diag=KB.SINGULAR_DIAG, scale=1.0)
    x = _zeros(n)
    assert jacobi.solve(b, x, maxiter=500).status == 0                   # the matrix is regular, and its diagonal is usable
    for nb in KB.BLOCKS:
        solver = whip.StencilSolver(op, diag=KB.SINGULAR_DIAG, scale=1.0, preconditioner=whip.BlockJacobi(nb))
        x = _t(x0)
        info = solver.solve(b, x)
        assert info.status == KR.DIAGONAL and info.iterations == 0 and _same_bits(x.cpu().numpy(), x0), (nb, info)
        solver.enqueue(b, x, 5)                                          # what is enqueued behind the stop leaves x alone
        assert solver.info().status == KR.DIAGONAL and _same_bits(x.cpu().numpy(), x0)
        solver.close()
    jacobi.close(); op.close()
    # a NaN inside a diagonal block
    sy = KR.system("random-n130")
    st = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in sy["st"].items()}
    st["own"][0, 70] = float("nan")
    st["own_mask"][70] = True
    op = whip.StencilOperator.from_coefficients(_t(st["hoods"]), _t(st["nk"]), _t(st["slots"]), 130, own=_t(st["own"]), own_mask=_t(st["own_mask"]))
    solver = whip.StencilSolver(op, diag=_t(sy["diag"]), scale=sy["scale"], preconditioner=whip.BlockJacobi(16))
    b, x0 = _t(sy["b"]), KR.guess(130)
    x = _t(x0)
    info = solver.solve(b, x)
    assert info.status == KR.DIAGONAL and info.iterations == 0 and _same_bits(x.cpu().numpy(), x0)
    solver.close(); op.close()
    # an empty slice under a zero diagonal: blocks of zeros
    st, op = _structure(whip, 130)
    rows_empty = np.asarray(st["nk"][64:128]) == 0
    assert rows_empty.all()
    solver = whip.StencilSolver(op, diag=0.0, scale=1.0, preconditioner=whip.BlockJacobi(32))
    x = _t(x0)
    info = solver.solve(b, x)
    assert info.status == KR.DIAGONAL and info.iterations == 0 and _same_bits(x.cpu().numpy(), x0)
    solver.close(); op.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------

def test_refusals(wlsqm):
    import torch
    import wlsqm.hip as whip
    n = 130
    st, op = _structure(whip, n, seed=5)
    solver = whip.StencilSolver(op, diag=2.0, preconditioner=whip.BlockJacobi(8))
    f64 = dict(dtype=torch.float64, device="cuda")
    v, out, both = torch.ones(n, **f64), torch.zeros(n, **f64), torch.zeros(2 * n, **f64)
    for bad_v, bad_out, message in ((both[:n], both[n - 1:2 * n - 1], "v overlaps out"), (v.float(), out, "expected 'float64'.*argument v"),
                                    (v.cpu(), out, "argument v must be a device"), (v, both[:n + 1], "out must be a contiguous.*shape \\(130,\\)"),
                                    (both[::2], out, "v must be a contiguous.*strides \\(2,\\)"), (v, out[None], "wrong number of dimensions"),
                                    (v, solver._planes[:n], "out overlaps the preconditioner's blocks")):
        with pytest.raises(ValueError, match=message):
            solver.precondition(bad_v, out=bad_out)
    assert torch.isfinite(solver.precondition(v, out=out)).all()         # the solver is none the worse
    with pytest.raises(ValueError, match="block must be 8, 16 or 32"):
        whip.BlockJacobi(12)
    jacobi = whip.StencilSolver(op, diag=2.0)
    for call in (jacobi.refresh, lambda: jacobi.precondition(v), jacobi.preconditioner_blocks):
        with pytest.raises(ValueError, match="belongs to a BlockJacobi preconditioner"):
            call()
    solver.close()
    with pytest.raises(RuntimeError, match="the stencil solver has been closed"):
        solver.precondition(v)
    jacobi.close(); op.close()
