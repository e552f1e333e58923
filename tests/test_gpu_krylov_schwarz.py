"""GPU tests of the overlapping blocks (wlsqm.hip.OverlappingBlocks, csrc/krylov.hip's krylov_schwarz_* kernels).

  1. the index table equal to tests/_krylov_schwarz_ref.py's, entry for entry; W and the transposed plane of EVERY block (a sample of
     blocks at 65 537 rows only) row by row against the numpy statement on the operator's own values, in the unit of section 19 (rows
     eps kappa_inf(A_B) |z|_inf per block) within 4 STATEMENT_RATIO, and against mpmath on the blocks that the host test sampled for
     that constant: the small systems, and square random structures of 1, 63, 64, 65, 300 and 65 537 rows, with 8 / 32, 16 / 32,
     8 / 64, 16 / 64 and 32 / 64; the columns at a -1 exactly zero; precondition(v), forward and transposed, against the reference's P.
     n = 130 leaves a last block of 2 rows and sets that reach into another slice; one block holds all of 20 rows.
  2. solves by the criteria of tests/test_gpu_krylov.py against the reference recurrences with the reference's P, both methods; the two
     3D systems at tau 1 with 32 / 64; BlockJacobi(16) printed beside;
  3. a transposed solve, and dL/db through differentiable_stencil_solve;
  4. bit for bit: twice, solve against enqueue, eager against a captured update + enqueue, refresh=False;
  5. statuses, never a fault;  6. the other preconditioners are untouched.
"""
import numpy as np
import pytest

import _krylov_block_ref as KB
import _krylov_ref as KR
import _krylov_schwarz_ref as SW
import _stencil_ref as R
from _device_helpers import bits, dev as _t, nan as _nan, same_bits as _same_bits, wlsqm  # noqa: F401 (fixture)
from test_gpu_krylov import _build

pytestmark = pytest.mark.gpu

F = 4.0 * SW.STATEMENT_RATIO


def _zeros(n):
    import torch
    return torch.zeros(n, dtype=torch.float64, device="cuda")


_made = {}
_squares = {}


def _system(name):
    """The system `name` on the device and what the tests share about it, computed once and left unchanged: the rows and the dense M
    from the operator's own values, and (lazily, per configuration) the reference's table, W and dense P."""
    if name not in _made:
        import wlsqm.hip as whip
        sy = SW.system(name)
        op, args = _build(whip, sy)
        slots, own = op.coefficients()
        rows = SW.rows_of_system(sy, slots.cpu().numpy(), own.cpu().numpy())
        M = SW.dense_of_rows(rows, sy["diag"], sy["scale"])
        _made[name] = dict(sy=sy, op=op, args=args, rows=rows, M=M, b=_t(sy["b"]), solvers={}, refs={})
    return _made[name]


def _reference(m, cfg):
    if cfg not in m["refs"]:
        sy = m["sy"]
        ref = SW.build_ref(m["rows"], sy["diag"], sy["scale"], *cfg)
        assert ref["usable"].all()
        ref["P"] = SW.dense_p(ref["table"], ref["W"], sy["n"])
        ref["PT"] = SW.dense_p(ref["table"], ref["WT"], sy["n"])
        m["refs"][cfg] = ref
    return m["refs"][cfg]


def _solver(m, pc, method="bicgstab"):
    import wlsqm.hip as whip
    if (pc, method) not in m["solvers"]:
        p = whip.OverlappingBlocks(*pc) if isinstance(pc, tuple) else whip.BlockJacobi(pc) if isinstance(pc, int) else pc
        m["solvers"][pc, method] = whip.StencilSolver(m["op"], preconditioner=p, method=method, **m["args"])
    return m["solvers"][pc, method]


def _checked(n, block):
    """The blocks whose W is compared with the reference: every one, but at 65 537 rows the first and last 16, the middle one and 200
    others (the numpy statement of every block would take a minute there)."""
    nblocks = (n + block - 1) // block
    if n <= 2000:
        return list(range(nblocks))
    rng = np.random.default_rng([53, block])
    return sorted(set(range(16)) | set(range(nblocks - 16, nblocks)) | {nblocks // 2} | set(rng.integers(0, nblocks, 200).tolist()))


def _held(what, solver, rows, diag, scale, n, cfg, whip):
    """The table against the reference's; W and the transposed plane of every block, row by row, against the numpy statement on the
    operator's own values, and on sampled() against mpmath, both within 4 STATEMENT_RATIO in section 19's unit; the -1 columns, the rows
    beyond a cut block and the corner that the two planes share; precondition(v), forward and transposed, against the reference's P."""
    block, nrows = cfg
    table, W = (t.cpu().numpy() for t in solver.preconditioner_overlapping_blocks())
    assert whip.last_kernel() == "krylov-schwarz-build"
    want = SW.sets_ref(SW.columns_of(rows), n, block, nrows)
    assert table.dtype == np.int32 and table.shape == want.shape and np.array_equal(table, want), what
    table_t, WT = (t.cpu().numpy() for t in solver.preconditioner_overlapping_blocks(transpose=True))
    assert np.array_equal(table_t, table) and W.shape == WT.shape == (want.shape[0], block, nrows)
    assert np.isfinite(W).all() and np.isfinite(WT).all()
    which = _checked(n, block)
    assert {B for B, _ in SW.sampled(n, block, nrows)} <= set(which)
    ref = SW.build_ref(rows, diag, scale, block, nrows, blocks=which, table=want)
    assert ref["usable"].all()
    gap, at, transposed = SW.worst_gap(ref, W[which], WT[which], n)
    ratio = SW.worst_ratio(ref, W[which], WT[which], n)
    ratio_ref = SW.worst_ratio(ref, ref["W"], ref["WT"], n)
    print("%s %d / %d: %d blocks against the numpy statement: worst %.4f (block %d%s); against mpmath on the sample: %.4f (the numpy "
          "statement's %.4f); bound %.4f; worst kappa_inf %.3g"
          % (what, block, nrows, len(which), gap, at, ", transposed" if transposed else "", ratio, ratio_ref, F,
             max(KB.kappa_inf(A) for A in ref["A"])))
    assert gap <= F, (what, cfg, gap, at, transposed)
    assert ratio <= F, (what, cfg, ratio)
    nblocks = want.shape[0]
    for B in range(nblocks):
        cnt = min(block, n - B * block)
        pad = want[B] < 0
        assert not W[B][:, pad].any() and not WT[B][:, pad].any(), (what, B, "a column at a -1 is not 0.0")
        assert not W[B, cnt:].any() and not WT[B, cnt:].any(), (what, B, "a row beyond the block is not 0.0")
        assert _same_bits(WT[B, :cnt, :cnt], W[B, :cnt, :cnt].T), (what, B, "the planes do not share their corner")
    if n > 2000:
        return table, W
    # precondition(v) against the reference's P: the product's own bound, and what W may differ by (F units per block)
    v = np.random.default_rng([71, n]).standard_normal(n)
    for transpose, Wr in ((False, ref["W"]), (True, ref["WT"])):
        P = SW.dense_p(want, Wr, n)
        out = _nan(n)
        z = solver.precondition(_t(v), out=out, transpose=transpose)
        assert z is out and whip.last_kernel() == "krylov-schwarz-apply"
        room = R.gamma(nrows + 2) * (np.abs(P) @ np.abs(v)) + 1e-300
        for k, B in enumerate(which):
            cnt = min(block, n - B * block)
            g = np.where(want[B] >= 0, v[np.maximum(want[B], 0)], 0.0)
            A = ref["A"][k].T if transpose else ref["A"][k]
            inv = ref["inv"][k].T if transpose else ref["inv"][k]
            room[B * block:B * block + cnt] += F * nrows * SW.EPS * KB.kappa_inf(A) * np.abs(inv @ g).max()
        err = np.abs(z.cpu().numpy() - P @ v)
        assert np.all(err <= room), (what, transpose, (err / room).max())
    return table, W


# ---- 1. the table and W --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", SW.CONFIGS)
@pytest.mark.parametrize("name", SW.W_SYSTEMS)
def test_table_and_w_against_the_reference(wlsqm, name, cfg):
    import wlsqm.hip as whip
    m = _system(name)
    sy, n = m["sy"], m["sy"]["n"]
    table, W = _held(name, _solver(m, cfg), m["rows"], sy["diag"], sy["scale"], n, cfg, whip)
    assert n - (table.shape[0] - 1) * cfg[0] == 2                        # a last block of 2 rows
    if sy["kind"] != "random":                                           # a block whose extension lies in another slice
        ext = table[:, cfg[0]:]
        first = (np.arange(table.shape[0]) * cfg[0])[:, None]
        assert ((ext >= 0) & (ext // 64 != first // 64)).any()


def _square(n):
    if n not in _squares:
        import wlsqm.hip as whip
        st, rows, d, c = SW.square_system(n)
        op = whip.StencilOperator.from_coefficients(_t(st["hoods"]), _t(st["nk"]), _t(st["slots"]), n, own=_t(st["own"]), own_mask=_t(st["own_mask"]))
        _squares[n] = (st, rows, d, c, op)
    return _squares[n]


@pytest.mark.parametrize("cfg", SW.CONFIGS)
@pytest.mark.parametrize("n", SW.SIZES + (20,))
def test_w_on_square_structures(wlsqm, n, cfg):
    """Empty rows, an empty slice, a last slice of one row, columns named twice, sets shorter than `rows`, more than one workgroup of the
    apply, 65 537 rows (a sample of blocks); and at n = 1 and n = 20 one set that holds every row: P is M^-1."""
    import wlsqm.hip as whip
    st, rows, d, c, op = _square(n)
    solver = whip.StencilSolver(op, diag=_t(d), scale=c, preconditioner=whip.OverlappingBlocks(*cfg))
    L = wlsqm._binding.lib()
    nblocks = (n + cfg[0] - 1) // cfg[0]
    assert solver.memory_used() == L.wlsqm_hip_krylov_workspace_bytes(n) + L.wlsqm_hip_krylov_schwarz_bytes(n, *cfg) + 4 * nblocks * cfg[1]
    _held("n = %d" % n, solver, rows, d, c, n, cfg, whip)
    b = np.random.default_rng([97, n]).standard_normal(n)
    M = SW.dense_of_rows(rows, d, c) if n <= 300 else None
    for method in SW.METHODS:
        s2 = whip.StencilSolver(op, diag=_t(d), scale=c, preconditioner=whip.OverlappingBlocks(*cfg), method=method)
        x = _zeros(n)
        info = s2.solve(_t(b), x, rtol=KR.RTOL, maxiter=60)
        assert whip.last_kernel() == ("krylov-schwarz-l2-update" if method == "bicgstab2" else "krylov-schwarz-update")
        out, _, _ = s2.product(x)
        true = np.linalg.norm(b - out.cpu().numpy())
        print("n %d %d / %d %s: %s, true residual %.3e" % ((n,) + cfg + (method, info, true)))
        assert info.status == KR.CONVERGED and true <= 4 * KR.RTOL * np.linalg.norm(b)
        if M is not None:
            assert np.linalg.norm(b - M @ x.cpu().numpy()) <= 4 * KR.RTOL * np.linalg.norm(b)
        if n <= cfg[0]:                                                  # one block, every row in it: one iteration, or one cycle
            assert info.iterations == (2 if method == "bicgstab2" else 1)
        s2.close()
    solver.close()


# ---- 2. solves ------------------------------------------------------------------------------------------------------------------------------

def _held_to_the_reference(m, cfg, x, info, method, cap, what, error=True, transpose=False):
    M, b = (np.ascontiguousarray(m["M"].T) if transpose else m["M"]), m["sy"]["b"]
    ref = _reference(m, cfg)
    xr, its_r, st_r, hist = SW.solve_ref(M, b, ref["PT"] if transpose else ref["P"], method, cap=cap)
    assert st_r == KR.CONVERGED, (what, st_r, its_r)
    stop = KR.RTOL * np.linalg.norm(b)
    gap = abs(np.linalg.norm(b - M @ xr) - hist[-1])
    true = np.linalg.norm(b - M @ x)
    print("%s: iterations %d (reference %d, cap %d), recursive %.3e true %.3e stop %.3e gap %.3e"
          % (what, info.iterations, its_r, cap, info.residual, true, stop, gap))
    assert info.status == KR.CONVERGED, (what, info)
    assert 0 < info.iterations <= cap, (what, info)                      # the cap is twice the reference's count on the oracle's values
    assert info.residual <= stop
    assert true <= stop + 8 * gap, (what, true, stop, gap)
    if error:
        xstar, kappa = np.linalg.solve(M, b), np.linalg.cond(M)
        err = np.linalg.norm(x - xstar) / np.linalg.norm(xstar)
        print("%s: error %.3e bound %.3e" % (what, err, kappa * true / np.linalg.norm(b)))
        assert err <= kappa * true / np.linalg.norm(b) * (1 + 1e-6), (what, err)


def _blocks_beside(m, method, what):
    x = _zeros(m["sy"]["n"])
    info = _solver(m, 16, method).solve(m["b"], x, rtol=KR.RTOL, maxiter=3000, check_every=64)
    print("%s: BlockJacobi(16) beside: %s" % (what, info))


@pytest.mark.parametrize("name,cfg,method", SW.GPU_CASES)
def test_solve(wlsqm, name, cfg, method):
    import wlsqm.hip as whip
    m = _system(name)
    n, cap = m["sy"]["n"], SW.CAPS[name][cfg][method]
    x = _zeros(n)
    info = _solver(m, cfg, method).solve(m["b"], x, rtol=KR.RTOL, maxiter=cap)
    assert whip.last_kernel() == ("krylov-schwarz-l2-update" if method == "bicgstab2" else "krylov-schwarz-update")
    what = "%s %d / %d %s" % ((name,) + cfg + (method,))
    _held_to_the_reference(m, cfg, x.cpu().numpy(), info, method, cap, what)
    _blocks_beside(m, method, what)


@pytest.mark.parametrize("name,method", SW.HEADLINE_CASES)
def test_large_step_in_3d(wlsqm, name, method):
    cfg = SW.HEADLINE_GPU
    m = _system(name)
    n, cap = m["sy"]["n"], SW.HEADLINE[name][cfg][method]
    x = _zeros(n)
    info = _solver(m, cfg, method).solve(m["b"], x, rtol=KR.RTOL, maxiter=cap)
    what = "%s %d / %d %s" % ((name,) + cfg + (method,))
    # the error criterion wants kappa_2 of a 2000 x 2000 matrix: the residual criterion alone at that size
    _held_to_the_reference(m, cfg, x.cpu().numpy(), info, method, cap, what, error=n <= 1000)
    _blocks_beside(m, method, what)


# ---- 3. transposed solves and autograd -------------------------------------------------------------------------------------------------------

def test_transposed_solve_and_autograd(wlsqm):
    import wlsqm.hip as whip
    name, cfg, method, cap = SW.TRANSPOSED
    m = _system(name)
    n = m["sy"]["n"]
    solver = whip.StencilSolver(m["op"], preconditioner=whip.OverlappingBlocks(*cfg), method=method, **m["args"])
    before = solver.memory_used()
    x = _zeros(n)
    info = solver.solve(m["b"], x, rtol=KR.RTOL, maxiter=cap, transpose=True)
    _held_to_the_reference(m, cfg, x.cpu().numpy(), info, method, cap, "transposed", transpose=True)
    assert solver.memory_used() == before + 8 * (solver._planes.numel())  # the second plane
    assert solver.prepare_transpose() is False
    w = _t(np.random.default_rng(83).standard_normal(n))
    grads = []
    default = whip.StencilSolver(m["op"], **m["args"])
    for s in (solver, default):
        b = m["b"].clone().requires_grad_(True)
        xs = whip.differentiable_stencil_solve(s, b, rtol=KR.RTOL, maxiter=1000)
        (xs * w).sum().backward()
        assert whip.last_kernel().startswith("krylov-schwarz-l2-update" if s is solver else "krylov-update")
        grads.append(b.grad.cpu().numpy())
    diff, size, kappa = np.linalg.norm(grads[0] - grads[1]), np.linalg.norm(grads[1]), np.linalg.cond(m["M"])
    print("dL/db: the overlapping blocks against the default solver %.3e of %.3e, bound %.3e" % (diff, size, kappa * KR.RTOL * size))
    assert diff <= kappa * KR.RTOL * size
    solver.close(); default.close()


# ---- 4. bit for bit ----------------------------------------------------------------------------------------------------------------------------

def test_same_bits_twice_and_behind_the_stop(wlsqm):
    import torch
    name, cfg = "3D-tau1-n130", (16, 32)
    m = _system(name)
    for method in SW.METHODS:
        solver, b, n, cap = _solver(m, cfg, method), m["b"], m["sy"]["n"], SW.CAPS[name][cfg][method]
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
        solver.enqueue(b, x, k - 2)
        assert solver.info().status == KR.MAXITER and not torch.equal(bits(x), bits(runs[1][1]))


def _moving(whip, refresh, method, cfg=(16, 32)):
    name = "2D-tau0.25-n130"
    sy = KB.morton_system(name)
    n = sy["n"]
    rng = np.random.default_rng(41)
    SA, SB = sy["S"], sy["S"] + 0.05 * n ** -0.5 * rng.standard_normal(sy["S"].shape)
    S = _t(SA)
    op = whip.StencilOperator(2, 2, S, _t(sy["hoods"]), _t(sy["nk"]), _t(sy["knowns"]), _t(sy["wm"]), _t(sy["rows"]))
    solver = whip.StencilSolver(op, diag=sy["diag"], scale=sy["scale"], preconditioner=whip.OverlappingBlocks(*cfg, refresh=refresh), method=method)
    return sy, n, SA, SB, S, op, solver


@pytest.mark.parametrize("method", SW.METHODS)
def test_capture_behind_update(wlsqm, method):
    import torch
    import wlsqm.hip as whip
    sy, n, SA, SB, S, op, solver = _moving(whip, True, method)
    b, x0 = _t(sy["b"]), _t(KR.guess(n))
    x = _nan(n)
    iters = 20                                                           # a count to enqueue, not a bound: the solves stop long before
    table = solver._table.clone()

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
    assert torch.equal(solver._table, table)                             # an update never touches the sets
    solver.close(); op.close()


def test_refresh_false_keeps_p_until_refresh(wlsqm):
    import torch
    import wlsqm.hip as whip
    sy, n, SA, SB, S, op, solver = _moving(whip, False, "bicgstab")
    b, x0 = _t(sy["b"]), _t(KR.guess(n))
    x = _nan(n)

    def step():
        x.copy_(x0)
        op.update(S, check=False)
        solver.enqueue(b, x, 20)

    planes = lambda: solver.preconditioner_overlapping_blocks()[1]
    step()                                                               # the first start builds P
    W_a, info_a = planes(), solver.info()
    S.copy_(_t(SB))
    step()
    stale, info_stale = x.clone(), solver.info()
    assert info_a.status == info_stale.status == 0                       # the old P on the moved operator still converges
    assert torch.equal(planes(), W_a)
    solver.refresh()
    W_b = planes()
    assert not torch.equal(W_b, W_a)
    step()
    assert solver.info().status == 0 and torch.equal(planes(), W_b)
    fresh = whip.StencilSolver(op, diag=sy["diag"], scale=sy["scale"], preconditioner=whip.OverlappingBlocks(16, 32))
    y = x0.clone()
    fresh.enqueue(b, y, 20)
    assert fresh.info() == solver.info() and torch.equal(bits(y), bits(x))
    assert not torch.equal(bits(stale), bits(x))
    fresh.close(); solver.close(); op.close()


# ---- 5. statuses, never a fault -------------------------------------------------------------------------------------------------------------

def test_statuses_without_a_fault(wlsqm):
    import wlsqm.hip as whip
    m = _system("random-n130")
    n, b = m["sy"]["n"], m["b"]
    x0 = KR.guess(n)
    cfg = (32, 64)
    for method in SW.METHODS:
        solver = _solver(m, cfg, method)
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
        solver.enqueue(bn, x, 6)
        assert solver.info().status == KR.NONFINITE and _same_bits(x.cpu().numpy(), x0)
        x = _zeros(n)
        assert solver.solve(b, x, maxiter=SW.CAPS["random-n130"][cfg][method]).status == KR.CONVERGED
    # an extended block with two equal rows inside a regular matrix
    st = SW.singular_extended_structure()
    n = st["npoints"]
    op = whip.StencilOperator.from_coefficients(_t(st["hoods"]), _t(st["nk"]), _t(st["slots"]), n, own=_t(st["own"]), own_mask=_t(st["own_mask"]))
    b, x0 = _t(np.random.default_rng(89).standard_normal(n)), KR.guess(n)
    jacobi = whip.StencilSolver(op, diag=KB.SINGULAR_DIAG, scale=1.0)
    x = _zeros(n)
    assert jacobi.solve(b, x, maxiter=500).status == 0                   # the matrix is regular, and its diagonal is usable
    for method in SW.METHODS:
        solver = whip.StencilSolver(op, diag=KB.SINGULAR_DIAG, scale=1.0, preconditioner=whip.OverlappingBlocks(8, 32), method=method)
        assert solver._table[0].tolist() == list(range(32))
        x = _t(x0)
        info = solver.solve(b, x)
        assert info.status == KR.DIAGONAL and info.iterations == 0 and _same_bits(x.cpu().numpy(), x0), (method, info)
        solver.enqueue(b, x, 5)                                          # what is enqueued behind the stop leaves x alone
        assert solver.info().status == KR.DIAGONAL and _same_bits(x.cpu().numpy(), x0)
        solver.close()
    jacobi.close(); op.close()


def test_refusals(wlsqm):
    import wlsqm.hip as whip
    m = _system("random-n130")
    with pytest.raises(ValueError, match="an OverlappingBlocks preconditions one right-hand side at a time: nfields must be 1; got 2"):
        whip.StencilSolver(m["op"], preconditioner=whip.OverlappingBlocks(), nfields=2, **m["args"])
    with pytest.raises(ValueError, match="for coupled fields"):
        whip.StencilSystemSolver(m["op"], np.ones((1, 1, 1)), preconditioner=whip.OverlappingBlocks())
    with pytest.raises(ValueError, match="belongs to an OverlappingBlocks preconditioner"):
        _solver(m, 16).preconditioner_overlapping_blocks()
    with pytest.raises(ValueError, match="belongs to a BlockJacobi preconditioner"):
        _solver(m, (32, 64)).preconditioner_blocks()


# ---- 6. the other preconditioners are untouched ----------------------------------------------------------------------------------------------

def test_the_other_preconditioners_are_unchanged(wlsqm):
    """StencilSolver(op), preconditioner=None, BlockJacobi(16) and ApproximateInverse(): the same bits, workspace and kernel families
    whether or not a solver with an OverlappingBlocks on the same operator has run in between, with both methods."""
    import torch
    import wlsqm.hip as whip
    m = _system("2D-tau1-n130")
    n = m["sy"]["n"]
    L = wlsqm._binding.lib()
    total = int(m["op"]._m["total"])
    extra = {"jacobi": 0, None: 0, 16: L.wlsqm_hip_krylov_block_bytes(n, 16), "spai": L.wlsqm_hip_krylov_spai_bytes(n, total)}
    for method, ws, fam in (("bicgstab", L.wlsqm_hip_krylov_workspace_bytes(n),
                             ("krylov-update", "krylov-update", "krylov-update-block", "krylov-spai-update")),
                            ("bicgstab2", L.wlsqm_hip_krylov_l2_workspace_bytes(n),
                             ("krylov-l2-update", "krylov-l2-update", "krylov-l2-update-block", "krylov-spai-l2-update"))):
        for pc, family in zip(("jacobi", None, 16, "spai"), fam):
            got = []
            for between in (False, True):
                if between:
                    x = _zeros(n)
                    assert _solver(m, (32, 64), method).solve(m["b"], x, maxiter=100).status == 0
                p = whip.BlockJacobi(pc) if pc == 16 else whip.ApproximateInverse() if pc == "spai" else pc
                solver = whip.StencilSolver(m["op"], preconditioner=p, method=method, **m["args"])
                assert solver.memory_used() - extra[pc] == ws
                x = _zeros(n)
                info = solver.solve(m["b"], x, rtol=KR.RTOL, maxiter=400)
                assert whip.last_kernel() == family
                got.append((info, x))
                solver.close()
            assert got[0][0] == got[1][0] and got[0][0].status == 0 and torch.equal(bits(got[0][1]), bits(got[1][1]))
