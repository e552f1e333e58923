"""GPU tests of the sparse approximate inverse preconditioner (wlsqm.hip.ApproximateInverse, csrc/krylov.hip's krylov_spai_* kernels,
DESIGN.md section 22).

  1. Q against tests/_krylov_spai_ref.py on the operator's own values, row by row within 8 C0 eps cond_2(G_i) max |q_i| of the Gram
     statement (C0: what tests/test_krylov_spai_host.py measures between the two statements): the small systems, square random structures
     of every size at which the kernels take another path, rows of 64 stored entries; the dead slots exactly 0.0; the transposed planes
     the transpose bit for bit; precondition(v) = Q v by the product's own bound.  At 65 537 rows the reference runs on a sample of the
     rows (the first and last slices and a few hundred between): all of them would take a minute of numpy.
  2. solves by the criteria of tests/test_gpu_krylov.py against the reference recurrences with the reference's Q as the callable, both
     methods; the two 3D systems at tau 1; the iteration counts of BlockJacobi(16) printed beside;
  3. a transposed solve, and dL/db through differentiable_stencil_solve;
  4. bit for bit: twice, solve against enqueue, eager against a captured update + enqueue, refresh=False;
  5. statuses, never a fault; refusals;  6. the other preconditioners are untouched.
"""
import numpy as np
import pytest

import _krylov_block_ref as KB
import _krylov_l2_ref as L2
import _krylov_ref as KR
import _krylov_spai_ref as SP
import _stencil_ref as R
from _device_helpers import bits, dev as _t, nan as _nan, same_bits as _same_bits, wlsqm  # noqa: F401 (fixture)
from test_gpu_krylov import _build

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 300, 65537)
BAR = 8 * SP.C0


def _zeros(n):
    import torch
    return torch.zeros(n, dtype=torch.float64, device="cuda")


_made = {}


def _system(name):
    """The system `name` on the device and what the tests share about it, computed once and left unchanged: the dense M and the rows of M
    from the operator's own values, and (lazily) the reference's Q."""
    if name not in _made:
        import wlsqm.hip as whip
        sy = SP.system(name)
        op, args = _build(whip, sy)
        slots, own = op.coefficients()
        rows = SP.rows_of_system(sy, slots.cpu().numpy(), own.cpu().numpy())
        MR = SP.m_rows(rows, sy["diag"], sy["scale"])
        M = KR.dense_of(sy, op.to_sparse_csr(0).to_dense().cpu().numpy())
        _made[name] = dict(sy=sy, op=op, args=args, M=M, MR=MR, b=_t(sy["b"]), solvers={})
    return _made[name]


def _reference(m, gram=False):
    """The reference's rows of Q and its dense Q (the lstsq statement's), once; the Gram statement with them where a test holds rows to it."""
    if "ref" not in m or (gram and "gram" not in m["ref"][0]):
        m["ref"] = SP.approximate_inverse_ref(m["MR"], gram=gram)
        m["Q"] = SP.dense_q(m["ref"], m["sy"]["n"])
    return m["ref"]


def _solver(m, pc, method="bicgstab"):
    import wlsqm.hip as whip
    if (pc, method) not in m["solvers"]:
        p = whip.ApproximateInverse() if pc == "spai" else whip.BlockJacobi(pc) if isinstance(pc, int) else pc
        m["solvers"][pc, method] = whip.StencilSolver(m["op"], preconditioner=p, method=method, **m["args"])
    return m["solvers"][pc, method]


def _device_rows(solver, nk, own_mask):
    """Row i of the device's Q slot by slot: [qd_i, the nk_i neighbour slots, the own slot where the row has one]."""
    qd, slots, own = (t.cpu().numpy() for t in solver.preconditioner_coefficients())
    return [np.r_[qd[i], slots[i, :nk[i]], own[i:i + 1] if own_mask[i] else []] for i in range(len(nk))]


def _held_rows(what, ref, got, rows):
    worst = worst_ls = 0.0
    for row, i in zip(ref, rows):
        q = got[i]
        assert len(q) == len(row["gram"]) and row["usable"], (what, i)
        assert all(q[k] == 0.0 for k, ok in enumerate(row["live"]) if not ok), (what, i, "a dead slot is not 0.0")
        worst, worst_ls = max(worst, SP.gap(row, q)), max(worst_ls, SP.gap(row, row["lstsq"]))
    print("%s: %d rows, worst |q - Gram statement| %.3f eps cond max|q| (bar %.0f); the lstsq statement's %.3f; cond_2(G) up to %.3g"
          % (what, len(rows), worst, BAR, worst_ls, max(r["cond"] for r in ref)))
    assert worst <= BAR, (what, worst)


def _transposed_and_applied(what, solver, n, lens_max):
    """preconditioner_matrix(transpose=True) is the transpose bit for bit; precondition(v) is Q v within gamma_{len + 2} |Q| |v|."""
    import torch
    Q = solver.preconditioner_matrix().to_dense()
    QT = solver.preconditioner_matrix(transpose=True).to_dense()
    assert torch.equal(QT, Q.T.contiguous()), what
    v = np.random.default_rng([71, n]).standard_normal(n)
    Qh = Q.cpu().numpy()
    room = R.gamma(lens_max + 3) * (np.abs(Qh) @ np.abs(v))
    for transpose, A in ((False, Qh), (True, Qh.T)):
        z = solver.precondition(_t(v), transpose=transpose).cpu().numpy()
        err = np.abs(z - A @ v)
        assert np.all(err <= (room if not transpose else R.gamma(n + 3) * (np.abs(A) @ np.abs(v))) + 1e-300), (what, transpose, err.max())
    return Qh


# ---- 1. Q against the reference ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SP.Q_SYSTEMS)
def test_q_against_the_reference(wlsqm, name):
    import wlsqm.hip as whip
    m = _system(name)
    sy, n = m["sy"], m["sy"]["n"]
    solver = _solver(m, "spai")
    nk = sy["st"]["nk"] if sy["kind"] == "random" else sy["nk"]
    own_mask = sy["st"]["own_mask"] if sy["kind"] == "random" else np.ones(n, bool)
    got = _device_rows(solver, nk, own_mask)
    assert whip.last_kernel() == "krylov-spai"
    _held_rows(name, _reference(m, gram=True), got, range(n))
    _transposed_and_applied(name, solver, n, int(nk.max()) + 1)


@pytest.mark.parametrize("n", SIZES)
def test_q_on_square_structures(wlsqm, n):
    """Empty rows, an empty slice, a last slice of one row, columns named twice, self columns and own entries (the dead slots), more than
    one workgroup of the apply, and 65 537 rows."""
    import wlsqm.hip as whip
    st = KR.square_structure(n, 9, seed=31)
    op = whip.StencilOperator.from_coefficients(_t(st["hoods"]), _t(st["nk"]), _t(st["slots"]), n, own=_t(st["own"]), own_mask=_t(st["own_mask"]))
    rows = R.rows_of(st["hoods"], st["nk"], st["slots"], st["own"], st["own_mask"], st["pts"])
    c = -0.75
    d = 1.0 + 1.5 * abs(c) * np.array([sum(abs(v[0]) for _, v in r) for r in rows])
    MR = SP.m_rows(rows, d, c)
    solver = whip.StencilSolver(op, diag=_t(d), scale=c, preconditioner=whip.ApproximateInverse())
    total = int(op._m["total"])
    assert solver.memory_used() == wlsqm._binding.lib().wlsqm_hip_krylov_workspace_bytes(n) + 8 * (n + (n + 63) // 64 + total)
    got = _device_rows(solver, st["nk"], st["own_mask"])
    if n <= 300:
        sample = list(range(n))
    else:
        rng = np.random.default_rng(53)
        sample = sorted(set(range(192)) | set(range(n - 130, n)) | set(rng.integers(0, n, 300).tolist()))
    ref = SP.approximate_inverse_ref(MR, sample, gram=True)
    if n >= 65:
        assert any(not all(r["live"]) for r in ref)                      # the structure has dead slots
    _held_rows("n = %d" % n, ref, got, sample)
    if n <= 300:
        _transposed_and_applied("n = %d" % n, solver, n, 10)
    # and a solve: the matrix is diagonally dominant
    b = np.random.default_rng([97, n]).standard_normal(n)
    for method in SP.METHODS:
        s2 = whip.StencilSolver(op, diag=_t(d), scale=c, preconditioner=whip.ApproximateInverse(), method=method)
        x = _zeros(n)
        info = s2.solve(_t(b), x, rtol=KR.RTOL, maxiter=60)
        out, _, _ = s2.product(x)
        true = np.linalg.norm(b - out.cpu().numpy())
        print("n %d %s: %s, true residual %.3e" % (n, method, info, true))
        assert info.status == KR.CONVERGED and true <= 4 * KR.RTOL * np.linalg.norm(b)
        s2.close()
    solver.close(); op.close()


def _wide_structure(n, K, seed, own=False):
    """Rows of K distinct neighbours each, none the row itself: K + 1 unknowns per row of Q.  own: an own entry behind them on two
    rows out of three (the third keeps K stored entries)."""
    rng = np.random.default_rng([seed, n, K])
    hoods = np.stack([(j + 1 + rng.permutation(n - 1)[:K]) % n for j in range(n)]).astype(np.int32)
    st = dict(hoods=hoods, nk=np.full(n, K, np.int32), slots=rng.standard_normal((1, n, K)))
    if own:
        st.update(own=rng.standard_normal((1, n)), own_mask=np.arange(n) % 3 != 2)
    return st


@pytest.mark.parametrize("own", (False, True))
def test_rows_of_64_stored_entries(wlsqm, own):
    """64 stored entries, and 65 where the 65th is the row's own entry (64 neighbours of an F-known point, the 2D order-4 shape)."""
    import wlsqm.hip as whip
    n, K = 200, 64
    st = _wide_structure(n, K, 59, own)
    more = dict(own=_t(st["own"]), own_mask=_t(st["own_mask"])) if own else {}
    op = whip.StencilOperator.from_coefficients(_t(st["hoods"]), _t(st["nk"]), _t(st["slots"]), n, **more)
    assert int(op._m["width"].max()) == (65 if own else 64)
    rows = R.rows_of(st["hoods"], st["nk"], st["slots"], st.get("own"), st.get("own_mask"), np.arange(n) if own else None)
    c = 0.25
    d = 1.0 + 1.5 * c * (np.abs(st["slots"][0]).sum(axis=1) + (np.abs(st["own"][0]) if own else 0.0))
    MR = SP.m_rows(rows, d, c)
    solver = whip.StencilSolver(op, diag=_t(d), scale=c, preconditioner=whip.ApproximateInverse())
    got = _device_rows(solver, st["nk"], st["own_mask"] if own else np.zeros(n, bool))
    sample = list(range(0, n, 5)) + [n - 1]
    _held_rows("64 stored entries", SP.approximate_inverse_ref(MR, sample, gram=True), got, sample)
    x = _zeros(n)
    b = np.random.default_rng(61).standard_normal(n)
    info = solver.solve(_t(b), x, rtol=KR.RTOL, maxiter=60)
    M = SP.dense_m(MR)
    assert info.status == KR.CONVERGED and np.linalg.norm(b - M @ x.cpu().numpy()) <= 4 * KR.RTOL * np.linalg.norm(b)
    solver.close(); op.close()
    if own:
        return
    # above the cap: the constructor refuses
    st = _wide_structure(80, 65, 59)
    op = whip.StencilOperator.from_coefficients(_t(st["hoods"]), _t(st["nk"]), _t(st["slots"]), 80)
    with pytest.raises(ValueError, match="rows of up to 64 neighbours; the operator's longest row has 65"):
        whip.StencilSolver(op, preconditioner=whip.ApproximateInverse())
    whip.StencilSolver(op, preconditioner=whip.BlockJacobi(16)).close()  # the others take it
    op.close()


# ---- 2. solves ------------------------------------------------------------------------------------------------------------------------------

def _held_to_the_reference(m, x, info, method, cap, what, error=True, transpose=False):
    M, b = (np.ascontiguousarray(m["M"].T) if transpose else m["M"]), m["sy"]["b"]
    _reference(m)
    Q = np.ascontiguousarray(m["Q"].T) if transpose else m["Q"]
    xr, its_r, st_r, hist = SP.solve_ref(M, b, Q, method, cap=cap)
    assert st_r == KR.CONVERGED, (what, st_r, its_r)
    stop = KR.RTOL * np.linalg.norm(b)
    gap = abs(np.linalg.norm(b - M @ xr) - hist[-1])
    true = np.linalg.norm(b - M @ x)
    print("%s: iterations %d (reference %d, cap %d), recursive %.3e true %.3e stop %.3e gap %.3e"
          % (what, info.iterations, its_r, cap, info.residual, true, stop, gap))
    assert info.status == KR.CONVERGED, (what, info)
    assert 0 < info.iterations <= cap, (what, info)
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


@pytest.mark.parametrize("name,method", SP.GPU_CASES)
def test_solve(wlsqm, name, method):
    import wlsqm.hip as whip
    m = _system(name)
    n, cap = m["sy"]["n"], SP.CAPS[name][method]
    x = _zeros(n)
    info = _solver(m, "spai", method).solve(m["b"], x, rtol=KR.RTOL, maxiter=cap)
    assert whip.last_kernel() == ("krylov-spai-l2-update" if method == "bicgstab2" else "krylov-spai-update")
    _held_to_the_reference(m, x.cpu().numpy(), info, method, cap, "%s %s" % (name, method))
    _blocks_beside(m, method, "%s %s" % (name, method))


@pytest.mark.parametrize("name,method", [(name, method) for name, caps in SP.HEADLINE.items() for method in caps])
def test_large_step_in_3d(wlsqm, name, method):
    m = _system(name)
    n, cap = m["sy"]["n"], SP.HEADLINE[name][method]
    x = _zeros(n)
    info = _solver(m, "spai", method).solve(m["b"], x, rtol=KR.RTOL, maxiter=cap)
    # the error criterion wants kappa_2 of a 2000 x 2000 matrix: the residual criterion alone at that size
    _held_to_the_reference(m, x.cpu().numpy(), info, method, cap, "%s %s" % (name, method), error=n <= 1000)
    _blocks_beside(m, method, "%s %s" % (name, method))


# ---- 3. transposed solves and autograd -------------------------------------------------------------------------------------------------------

def test_transposed_solve_and_autograd(wlsqm):
    import wlsqm.hip as whip
    name, cap = SP.TRANSPOSED
    m = _system(name)
    n = m["sy"]["n"]
    solver = whip.StencilSolver(m["op"], preconditioner=whip.ApproximateInverse(), method="bicgstab2", **m["args"])
    x = _zeros(n)
    info = solver.solve(m["b"], x, rtol=KR.RTOL, maxiter=cap, transpose=True)
    _held_to_the_reference(m, x.cpu().numpy(), info, "bicgstab2", cap, "transposed", transpose=True)
    w = _t(np.random.default_rng(83).standard_normal(n))
    grads = []
    default = whip.StencilSolver(m["op"], **m["args"])
    for s in (solver, default):
        b = m["b"].clone().requires_grad_(True)
        xs = whip.differentiable_stencil_solve(s, b, rtol=KR.RTOL, maxiter=1000)
        (xs * w).sum().backward()
        assert whip.last_kernel().startswith("krylov-spai-l2-update" if s is solver else "krylov-update")
        grads.append(b.grad.cpu().numpy())
    diff, size, kappa = np.linalg.norm(grads[0] - grads[1]), np.linalg.norm(grads[1]), np.linalg.cond(m["M"])
    print("dL/db: the approximate inverse against the default solver %.3e of %.3e, bound %.3e" % (diff, size, kappa * KR.RTOL * size))
    assert diff <= kappa * KR.RTOL * size
    assert solver.memory_used() > default.memory_used()
    solver.close(); default.close()


# ---- 4. bit for bit ----------------------------------------------------------------------------------------------------------------------------

def test_same_bits_twice_and_behind_the_stop(wlsqm):
    import torch
    name = "2D-tau1-n130"
    m = _system(name)
    for method in SP.METHODS:
        solver, b, n, cap = _solver(m, "spai", method), m["b"], m["sy"]["n"], SP.CAPS[name][method]
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


def _moving(whip, refresh, method):
    name = "2D-tau0.25-n130"
    sy = KB.morton_system(name)
    n = sy["n"]
    rng = np.random.default_rng(41)
    SA, SB = sy["S"], sy["S"] + 0.05 * n ** -0.5 * rng.standard_normal(sy["S"].shape)
    S = _t(SA)
    op = whip.StencilOperator(2, 2, S, _t(sy["hoods"]), _t(sy["nk"]), _t(sy["knowns"]), _t(sy["wm"]), _t(sy["rows"]))
    solver = whip.StencilSolver(op, diag=sy["diag"], scale=sy["scale"], preconditioner=whip.ApproximateInverse(refresh=refresh), method=method)
    return sy, n, SA, SB, S, op, solver


@pytest.mark.parametrize("method", SP.METHODS)
def test_capture_behind_update(wlsqm, method):
    import torch
    import wlsqm.hip as whip
    sy, n, SA, SB, S, op, solver = _moving(whip, True, method)
    b, x0 = _t(sy["b"]), _t(KR.guess(n))
    x = _nan(n)
    iters = 20                                                           # a count to enqueue, not a bound: the solves stop long before

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


def test_refresh_false_keeps_q_until_refresh(wlsqm):
    import torch
    import wlsqm.hip as whip
    sy, n, SA, SB, S, op, solver = _moving(whip, False, "bicgstab")
    b, x0 = _t(sy["b"]), _t(KR.guess(n))
    x = _nan(n)

    def step():
        x.copy_(x0)
        op.update(S, check=False)
        solver.enqueue(b, x, 20)

    dense = lambda: solver.preconditioner_matrix().to_dense()
    step()                                                               # the first start builds Q
    Q_a, info_a = dense(), solver.info()
    S.copy_(_t(SB))
    step()
    stale, info_stale = x.clone(), solver.info()
    assert info_a.status == info_stale.status == 0                       # the old Q on the moved operator still converges
    assert torch.equal(dense(), Q_a)
    solver.refresh()
    Q_b = dense()
    assert not torch.equal(Q_b, Q_a)
    step()
    assert solver.info().status == 0 and torch.equal(dense(), Q_b)
    fresh = whip.StencilSolver(op, diag=sy["diag"], scale=sy["scale"], preconditioner=whip.ApproximateInverse())
    y = x0.clone()
    fresh.enqueue(b, y, 20)
    assert fresh.info() == solver.info() and torch.equal(bits(y), bits(x))
    assert not torch.equal(bits(stale), bits(x))
    fresh.close(); solver.close(); op.close()


# ---- 5. statuses, never a fault; refusals -----------------------------------------------------------------------------------------------------

def test_statuses_without_a_fault(wlsqm):
    import wlsqm.hip as whip
    m = _system("random-n130")
    n, b = m["sy"]["n"], m["b"]
    x0 = KR.guess(n)
    for method in SP.METHODS:
        solver = _solver(m, "spai", method)
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
        assert solver.solve(b, x, maxiter=SP.CAPS["random-n130"][method]).status == KR.CONVERGED
    # rows of zeros with diag = 0 (an empty slice): their Gram matrix is 0, the first pivot is not positive
    st = KR.square_structure(130, 9, seed=31)
    op = whip.StencilOperator.from_coefficients(_t(st["hoods"]), _t(st["nk"]), _t(st["slots"]), 130, own=_t(st["own"]), own_mask=_t(st["own_mask"]))
    assert (np.asarray(st["nk"][64:128]) == 0).all()
    for method in SP.METHODS:
        solver = whip.StencilSolver(op, diag=0.0, scale=1.0, preconditioner=whip.ApproximateInverse(), method=method)
        x = _t(x0)
        info = solver.solve(b, x)
        assert info.status == KR.DIAGONAL and info.iterations == 0 and _same_bits(x.cpu().numpy(), x0), (method, info)
        Q = solver.preconditioner_matrix().to_dense().cpu().numpy()
        assert np.isfinite(Q).all() and not Q[64:128].any()
        solver.close()
    op.close()


def test_refusals(wlsqm):
    import wlsqm.hip as whip
    m = _system("random-n130")
    with pytest.raises(ValueError, match="an ApproximateInverse preconditions one right-hand side at a time: nfields must be 1; got 2"):
        whip.StencilSolver(m["op"], preconditioner=whip.ApproximateInverse(), nfields=2, **m["args"])
    with pytest.raises(ValueError, match="preconditioner must be 'jacobi' or None"):
        whip.StencilSolver(m["op"], preconditioner="spai", **m["args"])
    with pytest.raises(ValueError, match="belongs to an ApproximateInverse preconditioner"):
        _solver(m, 16).preconditioner_matrix()
    with pytest.raises(ValueError, match="belongs to a BlockJacobi preconditioner"):
        _solver(m, "spai").preconditioner_blocks()


# ---- 6. the other preconditioners are untouched ----------------------------------------------------------------------------------------------

def test_the_other_preconditioners_are_unchanged(wlsqm):
    """StencilSolver(op), preconditioner=None and BlockJacobi(16): the same bits, workspace and kernel families whether or not a solver
    with an ApproximateInverse on the same operator has run in between, with both methods."""
    import torch
    import wlsqm.hip as whip
    m = _system("2D-tau0.25-n130")
    n = m["sy"]["n"]
    L = wlsqm._binding.lib()
    for method, ws, fam in (("bicgstab", L.wlsqm_hip_krylov_workspace_bytes(n), ("krylov-update", "krylov-update", "krylov-update-block")),
                            ("bicgstab2", L.wlsqm_hip_krylov_l2_workspace_bytes(n), ("krylov-l2-update", "krylov-l2-update", "krylov-l2-update-block"))):
        for pc, family in zip(("jacobi", None, 16), fam):
            got = []
            for between in (False, True):
                if between:
                    x = _zeros(n)
                    assert _solver(m, "spai", method).solve(m["b"], x, maxiter=100).status == 0
                solver = whip.StencilSolver(m["op"], preconditioner=whip.BlockJacobi(pc) if pc == 16 else pc, method=method, **m["args"])
                assert solver.memory_used() - (0 if pc != 16 else L.wlsqm_hip_krylov_block_bytes(n, 16)) == ws
                x = _zeros(n)
                info = solver.solve(m["b"], x, rtol=KR.RTOL, maxiter=400)
                assert whip.last_kernel() == family
                got.append((info, x))
                solver.close()
            assert got[0][0] == got[1][0] and got[0][0].status == 0 and torch.equal(bits(got[0][1]), bits(got[1][1]))
