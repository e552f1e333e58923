"""GPU tests of the block-Jacobi preconditioner over points of the coupled solves (wlsqm.hip.PointBlockJacobi, csrc/krylov.hip's
krylov_system_blocks_kernel, krylov_system_update_block_kernel and krylov_system_precondition_kernel).

  1. the blocks and their application on random square structures of 1, 15, 16, 17, 63, 64, 65, 130 and 300 points (empty rows, an
     empty slice from 130 on) for every m, every NB, R < NB, blocks that cross a slice boundary (3, 5, 7 and 10 points from 65 points
     on) and a cut last block, both kinds of table and the three forms of diag:
       - _matrix_blocks() (a check hook), the gathered entries, against the dense statement in exact arithmetic within 4 nop eps of the magnitudes of
         their terms (at the small sizes bit for bit tests/_krylov_system_block_ref.block_statement);
       - preconditioner_blocks() inverted back against the same statement.  An inverse that precondition() holds to f NB eps kappa of
         the truth is B^-1 + E with |E|_inf <= f NB eps kappa |B^-1|_inf, and (B^-1 + E)^-1 = B - B E B to first order, so inverting
         back moves an entry by at most (f + 1) NB eps kappa_inf(B)^2 |B|_inf (the + 1: numpy's own inversion); that allowance comes on
         top of the 4 nop eps of the magnitudes, which alone no inverse of a block with kappa > 1 can meet;
       - precondition(v) and its transpose against the mpmath block solve within 4 STATEMENT_RATIO in the unit NB eps kappa_inf |z|_inf;
       - the rows and columns from R on, what the cut last block leaves over and the blocks behind the last hold the exact identity;
  2. for m = 2 and 4 with R = NB: the blocks and the iteration count of a StencilSolver with BlockJacobi(R) on the flattened matrix();
  3. solves by section 17's criteria against _krylov_block_ref.bicgstab_block_ref on the library's own values, transposed and
     per-point systems included, a non-zero start and a diag tensor; 4. the gain over the scalar diagonal;
  5. bit for bit: twice, check_every=1 against one enqueue, eager against a captured op.update + enqueue, refresh=False;
  6. status 4 without a fault; 7. autograd; 8. a Jacobi system solver and a scalar BlockJacobi solver beside it keep their bits."""
import numpy as np
import pytest

import _krylov_block_ref as KB
import _krylov_ref as KR
import _krylov_system_block_ref as BR
import _krylov_system_ref as SR
from _device_helpers import bits, dev as _t, nan as _nan, same_bits as _same_bits, wlsqm  # noqa: F401 (fixture)
from test_gpu_krylov_system import _operator

pytestmark = pytest.mark.gpu

F = 4.0 * BR.STATEMENT_RATIO
EPS = BR.EPS


def _zeros(n, m):
    import torch
    return torch.zeros((n, m), dtype=torch.float64, device="cuda")


# ---- 1. the blocks and their application ---------------------------------------------------------------------------------------------------

def _worst_ratio(blocks, z, z_true):
    """_krylov_block_ref.worst_ratio on blocks of R rows in the unit of the padded ones: NB eps kappa_inf(padded B) |z_true|_inf."""
    nblocks, rows, _ = blocks.shape
    nb = BR.nb_of(rows)
    padded = BR.pad_blocks(blocks)
    pad = nblocks * rows - len(z)
    zz, zt = np.r_[z, np.zeros(pad)].reshape(nblocks, rows), np.r_[z_true, np.zeros(pad)].reshape(nblocks, rows)
    worst = 0.0
    for B in range(nblocks):
        scale = nb * EPS * KB.kappa_inf(padded[B]) * np.abs(zt[B]).max()
        err = np.abs(zz[B] - zt[B]).max()
        if err > 0.0:
            worst = max(worst, err / scale)
    return worst


@pytest.mark.parametrize("m,points", [(m, p) for m, pts in BR.BLOCK_POINTS.items() for p in pts])
def test_blocks_and_their_application(wlsqm, m, points):
    import torch
    import wlsqm.hip as whip
    L = wlsqm._binding.lib()
    nop = SR.RANDOM_NOP[m]
    rows_of_block = m * points
    nb = BR.nb_of(rows_of_block)
    seen = set()
    for mm, n, p, form, point in BR.block_cases(m, points):
        seen.add((form, point))
        st, rows, coupling, diag = BR.block_case(n, m, form, point)
        if n >= 130:
            lens = np.array([len(r) for r in rows])
            assert lens.min() == 0 and np.all(lens[64:128] == 0)          # empty rows and an empty slice
        op = _operator(whip, st)
        solver = whip.StencilSystemSolver(op, _t(coupling) if point else coupling, diag=_t(diag) if form == "tensor" else diag,
                                          preconditioner=whip.PointBlockJacobi(points))
        assert (solver.block_points, solver.block_rows, solver.per_point) == (points, rows_of_block, point)
        lay = BR.layout(n, m, points)
        nblocks = lay["nblocks"]
        assert solver.memory_used() == L.wlsqm_hip_krylov_system_workspace_bytes(n, m) + 8 * lay["doubles"]
        # the gathered entries
        exact, mag = BR.exact_blocks(rows, coupling, diag, points)
        G = solver._matrix_blocks()
        assert tuple(G.shape) == (nblocks, rows_of_block, rows_of_block) and whip.last_kernel() == "krylov-system-blocks"
        G = G.cpu().numpy()
        assert np.all(np.abs(G - exact) <= 4 * nop * EPS * mag), (n, form, point)
        statement = BR.block_statement(rows, coupling, diag, points)
        if n <= 65:
            assert _same_bits(G, statement), (n, form, point)
        # the inverses, inverted back
        W = solver.preconditioner_blocks()
        assert tuple(W.shape) == (nblocks, rows_of_block, rows_of_block) and whip.last_kernel() == "krylov-system-blocks"
        W = W.cpu().numpy()
        assert np.isfinite(W).all()
        back = np.linalg.inv(W)
        kappa = np.array([KB.kappa_inf(B) for B in statement])
        size = np.abs(statement).sum(axis=2).max(axis=1)
        room = 4 * nop * EPS * mag + ((F + 1.0) * nb * EPS * kappa ** 2 * size)[:, None, None]
        assert np.all(np.abs(back - statement) <= room), (n, form, point, float((np.abs(back - statement) / room).max()))
        # the plane itself: the identity from R on, in what the cut block leaves over and behind the last block
        plane = BR.blocks_of_plane(solver._planes.cpu().numpy(), n, m, points)
        assert plane.shape == (lay["nwaves"] * lay["per"], nb, nb)
        assert np.array_equal(plane[:nblocks, :rows_of_block, :rows_of_block], W)
        rest = plane.copy()
        rest[:nblocks, :rows_of_block, :rows_of_block] = np.eye(rows_of_block)
        assert np.all(rest == np.eye(nb)[None])
        cut = (n - (nblocks - 1) * points) * m
        over = W[-1].copy()
        over[:cut, :cut] = np.eye(cut)
        assert np.all(over == np.eye(rows_of_block))
        # the application against the mpmath block solve
        rng = np.random.default_rng([71, n, m, points])
        v = rng.standard_normal((n, m)) * 10.0 ** rng.integers(-2, 3, (n, m))
        out = _nan(n, m)
        z = solver.precondition(_t(v), out=out)
        assert z is out and whip.last_kernel() == "krylov-system-precondition"
        zn = z.cpu().numpy()
        truth, truth_t = BR.mp_block_solves(statement, v.reshape(-1))
        ratio = _worst_ratio(statement, zn.reshape(-1), truth)
        zt = solver.precondition(_t(v), transpose=True).cpu().numpy()
        ratio_t = _worst_ratio(np.ascontiguousarray(statement.transpose(0, 2, 1)), zt.reshape(-1), truth_t)
        print("n %d m %d points %d %s %s: worst ratio %.3f, transposed %.3f (bound %.3f)"
              % (n, m, points, form, "per point" if point else "constant", ratio, ratio_t, F))
        assert np.isfinite(zn).all() and ratio <= F and ratio_t <= F
        WT = solver.preconditioner_blocks(transpose=True).cpu().numpy()
        assert _same_bits(WT, W.transpose(0, 2, 1))
        plane_t = BR.blocks_of_plane(solver._planes_t.cpu().numpy(), n, m, points)
        assert np.all(plane_t == plane.transpose(0, 2, 1))
        mixed = 8 * n * nop * m if point else 0                          # a per-point table's transposed product mixes into a plane
        assert solver.memory_used() == L.wlsqm_hip_krylov_system_workspace_bytes(n, m) + 16 * lay["doubles"] + mixed
        # precondition is these blocks applied: R terms with fma against numpy's sum of the same terms
        za = BR.apply_blocks(W, v)
        assert np.all(np.abs(za - zn) <= 2 * nb * EPS * BR.apply_blocks(np.abs(W), np.abs(v)))
        again = solver.precondition(_t(v))
        assert torch.equal(bits(again), bits(z))
        solver.close(); op.close()
    assert len(seen) == 6                                                # the three forms of diag with both kinds of table


# ---- 2. agreement with the scalar block preconditioner ---------------------------------------------------------------------------------

def _flattened(whip, system):
    """A StencilOperator of one plane from system.matrix(): the route that existed before."""
    import torch
    M = system.matrix()
    crow, col, val = M.crow_indices(), M.col_indices(), M.values()
    nrows = int(crow.shape[0]) - 1
    nk = crow[1:] - crow[:-1]
    K = int(nk.max())
    row = torch.repeat_interleave(torch.arange(nrows, device=col.device), nk)
    slot = torch.arange(col.shape[0], device=col.device) - crow[:-1][row]
    hoods = torch.zeros((nrows, K), dtype=torch.int32, device=col.device)
    slots = torch.zeros((1, nrows, K), dtype=torch.float64, device=col.device)
    hoods[row, slot] = col.to(torch.int32)
    slots[0, row, slot] = val
    return whip.StencilOperator.from_coefficients(hoods, nk.to(torch.int32), slots, nrows)


@pytest.mark.parametrize("m,points", [(2, 4), (2, 8), (2, 16), (4, 2), (4, 4), (4, 8)])
def test_agreement_with_the_scalar_block_preconditioner(wlsqm, m, points):
    import torch
    import wlsqm.hip as whip
    s = _system("random-m%d" % m)
    sy, n = s["sy"], s["sy"]["n"]
    rows_of_block = m * points
    assert rows_of_block == BR.nb_of(rows_of_block)
    system = whip.StencilSystemSolver(s["op"], s["coupling"], diag=s["diag"], preconditioner=whip.PointBlockJacobi(points))
    flat_op = _flattened(whip, system)
    flat = whip.StencilSolver(flat_op, diag=0.0, scale=1.0, preconditioner=whip.BlockJacobi(rows_of_block))
    W, Wf = system.preconditioner_blocks().cpu().numpy(), flat.preconditioner_blocks().cpu().numpy()
    assert W.shape == Wf.shape
    blocks = BR.point_blocks_of(s["M"], m, points)
    # each within f NB eps kappa of the true inverse, in the norm of the inverse: the sum of the two bounds
    room = np.array([2 * F * rows_of_block * EPS * KB.kappa_inf(B) * np.abs(np.linalg.inv(B)).sum(axis=1).max() for B in blocks])
    assert np.all(np.abs(W - Wf).max(axis=(1, 2)) <= room)
    x, xf = _zeros(n, m), torch.zeros(n * m, dtype=torch.float64, device="cuda")
    info = system.solve(s["b"], x, rtol=KR.RTOL, maxiter=100)
    info_f = flat.solve(s["b"].reshape(-1), xf, rtol=KR.RTOL, maxiter=100)
    print("m %d points %d: %d iterations, flattened BlockJacobi(%d) %d" % (m, points, info.iterations, rows_of_block, info_f.iterations))
    assert info.status == info_f.status == 0 and abs(info.iterations - info_f.iterations) <= 2
    system.close(); flat.close(); flat_op.close()


# ---- 3. solves --------------------------------------------------------------------------------------------------------------------------------

_made = {}


def _system(name):
    """The system `name` of tests/_krylov_system_block_ref.py on the device and what the tests share about it, computed once."""
    if name not in _made:
        import wlsqm.hip as whip
        sy = BR.system(name)
        if sy["kind"] == "random":
            op = _operator(whip, sy["st"])
        else:
            op = whip.StencilOperator(sy["dim"], sy["order"], _t(sy["S"]), _t(sy["hoods"]), _t(sy["nk"]), _t(sy["knowns"]), _t(sy["wm"]),
                                      _t(sy["rows"]))
        diag = _t(sy["diag"]) if np.ndim(sy["diag"]) == 3 else sy["diag"]
        coupling = _t(sy["coupling"]) if np.ndim(sy["coupling"]) == 4 else sy["coupling"]
        A = np.stack([op.to_sparse_csr(o).to_dense().cpu().numpy() for o in range(sy["nop"])])
        M = BR.dense_matrix(A, sy["coupling"], sy["diag"])
        _made[name] = dict(sy=sy, op=op, diag=diag, coupling=coupling, M=M, b=_t(sy["b"]), bflat=sy["b"].reshape(-1), solvers={})
    return _made[name]


def _solver(s, points):
    import wlsqm.hip as whip
    if points not in s["solvers"]:
        s["solvers"][points] = whip.StencilSystemSolver(s["op"], s["coupling"], diag=s["diag"], preconditioner=whip.PointBlockJacobi(points))
    return s["solvers"][points]


def _held_to_the_reference(M, b, m, points, x, info, cap, what, x0=None):
    """Section 17's criteria against the block-preconditioned reference on the same matrix (M^T for a transposed solve); flat vectors."""
    xr, its_r, st_r, hist = BR.solve_ref(M, b, m, points, x0=x0, cap=cap)
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


@pytest.mark.parametrize("key", BR.GPU_CASES, ids=lambda k: "%s-%d%s" % (k[0], k[1], "-T" if k[2] else ""))
def test_solve(wlsqm, key):
    import wlsqm.hip as whip
    name, points, transposed = key
    s = _system(name)
    sy = s["sy"]
    solver = _solver(s, points)
    assert solver.block_points == points
    cap = BR.CAPS[key]
    info = solver.solve(s["b"], rtol=KR.RTOL, maxiter=cap, transpose=transposed)
    assert whip.last_kernel() == "krylov-system-update-block"
    x = solver.x
    assert tuple(x.shape) == (sy["n"], sy["m"])
    M = np.ascontiguousarray(s["M"].T) if transposed else s["M"]
    _held_to_the_reference(M, s["bflat"], sy["m"], points, x.cpu().numpy().reshape(-1), info, cap, "%s %d points%s" % (name, points, " transposed" if transposed else ""))


def test_default_points(wlsqm):
    import wlsqm.hip as whip
    for m in (1, 2, 3, 4):
        s = _system("random-m%d" % m)
        solver = whip.StencilSystemSolver(s["op"], s["coupling"], diag=s["diag"], preconditioner=whip.PointBlockJacobi())
        assert (solver.block_points, solver.block_rows) == (16 // m, m * (16 // m))
        solver.close()


def test_solve_from_a_guess_with_a_diag_tensor(wlsqm):
    """A non-zero x0 on a system with a per-point diag tensor (random-m3) and on an elasticity system; the cap is the zero start's."""
    for name, points in (("random-m3", 5), ("elasticity-2D-n130", 8)):
        s = _system(name)
        sy = s["sy"]
        x0 = np.random.default_rng([67, sy["n"]]).standard_normal((sy["n"], sy["m"]))
        x = _t(x0)
        cap = BR.CAPS[name, points, False]
        solver = _solver(s, points)
        info = solver.solve(s["b"], x, rtol=KR.RTOL, maxiter=cap, check_every=3)
        assert solver.x is x
        _held_to_the_reference(s["M"], s["bflat"], sy["m"], points, x.cpu().numpy().reshape(-1), info, cap, name + " from a guess", x0=x0.reshape(-1))
    assert np.ndim(_system("random-m3")["sy"]["diag"]) == 3


# ---- 4. the gain --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,points", BR.GAIN)
def test_the_gain_over_the_scalar_diagonal(wlsqm, name, points):
    """The device's count is at most 1.25 (the reversed-order margin) times the blocks-to-Jacobi ratio of the reference — measured
    here on the library's own values, as tests/test_krylov_system_block_host.py measures it on the oracle's (96 / 213 in the
    rehearsal) — times the device's own Jacobi count in the same run."""
    import wlsqm.hip as whip
    s = _system(name)
    sy = s["sy"]
    ratio = BR.gain_ratio(s["M"], s["bflat"], sy["m"], points)
    jacobi = whip.StencilSystemSolver(s["op"], s["coupling"], diag=s["diag"])
    ij = jacobi.solve(s["b"], rtol=KR.RTOL, maxiter=2000)
    ib = _solver(s, points).solve(s["b"], rtol=KR.RTOL, maxiter=2000)
    print("%s: Jacobi %d iterations, %d points %d; the reference's ratio %.3f, the device's %.3f"
          % (name, ij.iterations, points, ib.iterations, ratio, ib.iterations / ij.iterations))
    assert ij.status == ib.status == 0
    assert (96 / 213) / 1.25 <= ratio <= (96 / 213) * 1.25
    assert ib.iterations <= 1.25 * ratio * ij.iterations
    jacobi.close()


# ---- 5. bit for bit -------------------------------------------------------------------------------------------------------------------------------

def test_same_bits_twice_and_behind_the_stop(wlsqm):
    import torch
    name, points = "elasticity-2D-n130", 8
    s = _system(name)
    solver, b, sy = _solver(s, points), s["b"], s["sy"]
    cap = BR.CAPS[name, points, False]
    runs = []
    for check_every in (8, 8, 1):
        x = _zeros(sy["n"], sy["m"])
        runs.append((solver.solve(b, x, maxiter=cap, check_every=check_every), x))
    assert runs[0][0] == runs[1][0] == runs[2][0] and runs[0][0].status == 0
    assert torch.equal(bits(runs[0][1]), bits(runs[1][1])) and torch.equal(bits(runs[0][1]), bits(runs[2][1]))
    k = runs[2][0].iterations
    x = _zeros(sy["n"], sy["m"])
    before = torch.cuda.memory_allocated()
    solver.enqueue(b, x, k + 5)                                          # the five behind the stop leave x and the scalars alone
    assert torch.cuda.memory_allocated() == before
    assert solver.info() == runs[2][0] and torch.equal(bits(x), bits(runs[2][1]))
    x = _zeros(sy["n"], sy["m"])
    solver.enqueue(b, x, k - 1)                                          # one too few: the early exit is not what made them agree
    assert solver.info().status == KR.MAXITER and solver.info().iterations == k - 1
    assert not torch.equal(bits(x), bits(runs[2][1]))


@pytest.mark.parametrize("point", [False, True], ids=["constant", "per-point"])
def test_capture_behind_update_and_refresh_false(wlsqm, point):
    """Eager against a captured op.update(S, check=False) + enqueue, replayed after S.copy_ and, per point, after coupling.copy_; a
    refresh=False solver keeps the old blocks bit for bit through the replay and still converges, and after refresh() its blocks,
    iterate and scalars are those of a refresh=True solver."""
    import torch
    import wlsqm.hip as whip
    sy = BR.system("point-elasticity-2D-n130" if point else "elasticity-2D-n130")
    n, m, points = sy["n"], sy["m"], 8
    rng = np.random.default_rng(41)
    SA, SB = sy["S"], sy["S"] + 0.02 * n ** -0.5 * rng.standard_normal(sy["S"].shape)
    CA = sy["coupling"]
    CB = CA * (1.0 + 0.1 * rng.uniform(-1.0, 1.0, n)) if point else CA
    S = _t(SA)
    coupling = _t(CA) if point else CA
    op = whip.StencilOperator(sy["dim"], sy["order"], S, _t(sy["hoods"]), _t(sy["nk"]), _t(sy["knowns"]), _t(sy["wm"]), _t(sy["rows"]))
    solver = whip.StencilSystemSolver(op, coupling, diag=sy["diag"], preconditioner=whip.PointBlockJacobi(points))
    kept = whip.StencilSystemSolver(op, coupling, diag=sy["diag"], preconditioner=whip.PointBlockJacobi(points, refresh=False))
    b, x0 = _t(sy["b"]), _t(rng.standard_normal((n, m)))
    x, xk = _nan(n, m), _nan(n, m)
    iters = 3 * BR.CAPS["elasticity-2D-n130", points, False]             # a count to enqueue, not a bound

    def step():
        x.copy_(x0)
        xk.copy_(x0)
        op.update(S, check=False)
        solver.enqueue(b, x, iters)
        kept.enqueue(b, xk, iters)

    def move(SX, CX):
        S.copy_(_t(SX))
        if point:
            coupling.copy_(_t(CX))

    step()
    at_a, info_a = x.clone(), solver.info()
    blocks_a = kept._planes.clone()
    assert torch.equal(bits(xk), bits(at_a)) and kept.info() == info_a   # the first start factors either way
    move(SB, CB)
    step()
    eager, info_b = x.clone(), solver.info()
    kept_b, kept_info_b = xk.clone(), kept.info()
    assert info_a.status == info_b.status == kept_info_b.status == 0 and not torch.equal(bits(eager), bits(at_a))
    assert torch.equal(bits(kept._planes), bits(blocks_a)) and not torch.equal(bits(solver._planes), bits(blocks_a))
    move(SA, CA)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        step()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(x), bits(at_a)) and solver.info() == info_a
    move(SB, CB)
    x.fill_(float("nan")); xk.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(x), bits(eager)) and solver.info() == info_b
    assert torch.equal(bits(kept._planes), bits(blocks_a))               # the old blocks, through the replay
    assert torch.equal(bits(xk), bits(kept_b)) and kept.info() == kept_info_b
    x.copy_(x0)
    assert solver.solve(b, x, maxiter=iters) == info_b and torch.equal(bits(x), bits(eager))
    assert kept.refresh() is kept and whip.last_kernel() == "krylov-system-blocks"
    assert torch.equal(bits(kept._planes), bits(solver._planes))
    xk.copy_(x0)
    assert kept.solve(b, xk, maxiter=iters) == info_b and torch.equal(bits(xk), bits(eager))
    assert torch.equal(bits(kept._ws[:16]), bits(solver._ws[:16]))
    # a transposed start inside a capture without the plane of the transposes: the operator's convention
    fresh = whip.StencilSystemSolver(op, coupling, diag=sy["diag"], preconditioner=whip.PointBlockJacobi(points))
    op.prepare_transpose()
    if not point:
        g2 = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="no transposed preconditioner blocks yet and the stream is capturing"):
            with torch.cuda.graph(g2, stream=torch.cuda.Stream()):
                fresh.enqueue(b, x, 2, transpose=True)
        torch.cuda.synchronize()
    assert fresh.prepare_transpose() is True and fresh.prepare_transpose() is False
    solver.close(); kept.close(); fresh.close(); op.close()


def test_set_coupling_and_a_changed_diag_are_seen_by_the_next_factor(wlsqm):
    import torch
    import wlsqm.hip as whip
    s = _system("random-m2")
    sy = s["sy"]
    n, m, points = sy["n"], sy["m"], 8
    diag = _t(sy["diag"])
    solver = whip.StencilSystemSolver(s["op"], sy["coupling"], diag=diag, preconditioner=whip.PointBlockJacobi(points))
    x1 = _zeros(n, m)
    first = solver.solve(s["b"], x1, maxiter=100)
    diag.mul_(1.5)
    solver.set_coupling(0.5 * sy["coupling"])
    x2 = _zeros(n, m)
    second = solver.solve(s["b"], x2, maxiter=100)
    fresh = whip.StencilSystemSolver(s["op"], 0.5 * sy["coupling"], diag=_t(1.5 * sy["diag"]), preconditioner=whip.PointBlockJacobi(points))
    x3 = _zeros(n, m)
    third = fresh.solve(s["b"], x3, maxiter=100)
    assert first.status == second.status == 0 and second == third
    assert torch.equal(bits(x2), bits(x3)) and not torch.equal(bits(x1), bits(x2))
    assert torch.equal(bits(solver._planes), bits(fresh._planes))
    solver.close(); fresh.close()


# ---- 6. status 4, never a fault ---------------------------------------------------------------------------------------------------------------

def test_statuses(wlsqm):
    import torch
    import wlsqm.hip as whip
    s = _system("random-m3")
    sy, solver = s["sy"], _solver(s, 5)
    n, mm = sy["n"], sy["m"]
    x = _zeros(n, mm)
    info = solver.solve(_zeros(n, mm), x)                                # b = 0 from x = 0: converged before the first iteration
    assert (info.status, info.iterations, info.residual) == (0, 0, 0.0) and torch.all(x == 0.0)
    x0 = np.random.default_rng(71).standard_normal((n, mm))
    x = _t(x0)
    info = solver.solve(s["b"], x, maxiter=0)
    assert (info.status, info.iterations) == (KR.MAXITER, 0) and _same_bits(x.cpu().numpy(), x0)
    bn = s["b"].clone()
    bn[3, 1] = float("nan")
    x = _t(x0)
    info = solver.solve(bn, x)
    assert info.status == KR.NONFINITE and info.iterations == 0 and _same_bits(x.cpu().numpy(), x0)
    # a point whose own 2 x 2 block is [[1, 1], [1, 1]] with points = 1, inside a regular M with a non-zero diagonal
    sp = BR.singular_point_system()
    op = _operator(whip, sp["st"])
    b = _t(sp["b"])
    M = SR.dense_matrix(np.stack([op.to_sparse_csr(0).to_dense().cpu().numpy()]), sp["coupling"], sp["diag"])
    assert np.array_equal(M[:2, :2], np.ones((2, 2)))
    assert SR.solve_ref(M, sp["b"].reshape(-1), "jacobi")[2] == KR.CONVERGED      # on the CPU: Jacobi's reference converges on it
    jacobi = whip.StencilSystemSolver(op, sp["coupling"], diag=sp["diag"])
    assert jacobi.solve(b, maxiter=2 * M.shape[0]).status == 0
    x0 = np.random.default_rng(73).standard_normal((sp["n"], 2))
    for points, status in ((1, KR.DIAGONAL), (2, 0)):                    # with 2 points the block of 4 rows is regular
        blocks = whip.StencilSystemSolver(op, sp["coupling"], diag=sp["diag"], preconditioner=whip.PointBlockJacobi(points))
        x = _t(x0)
        info = blocks.solve(b, x, maxiter=2 * M.shape[0])
        assert info.status == status, (points, info)
        if status == KR.DIAGONAL:
            assert info.iterations == 0 and _same_bits(x.cpu().numpy(), x0) and np.isnan(info.residual)
            x = _t(x0)
            info = blocks.solve(b, x, transpose=True)
            assert info.status == KR.DIAGONAL and info.iterations == 0 and _same_bits(x.cpu().numpy(), x0)
        blocks.close()
    jacobi.close(); op.close()
    # a NaN in one point's coefficients
    p = _system("point-random-m3")
    cp = p["coupling"].clone()
    rows = SR.rows_of_structure(p["sy"]["st"])
    at = next(i for i, r in enumerate(rows) if i >= 70 and any(c // 5 == i // 5 for c, _ in r))    # a point with an entry inside its block
    cp[1, 1, 0, at] = float("nan")
    nan_table = whip.StencilSystemSolver(p["op"], cp, diag=p["diag"], preconditioner=whip.PointBlockJacobi(5))
    x0 = np.random.default_rng(79).standard_normal((n, mm))
    x = _t(x0)
    info = nan_table.solve(p["b"], x)
    assert info.status == KR.DIAGONAL and info.iterations == 0 and _same_bits(x.cpu().numpy(), x0)
    nan_table.close()
    # an empty slice under a zero diag
    st, rows, coupling, diag = BR.block_case(130, 2, "float", False)
    op = _operator(whip, st)
    empty = whip.StencilSystemSolver(op, coupling, diag=0.0, preconditioner=whip.PointBlockJacobi(8))
    x0 = np.random.default_rng(83).standard_normal((130, 2))
    x = _t(x0)
    info = empty.solve(_t(np.ones((130, 2))), x)
    assert info.status == KR.DIAGONAL and info.iterations == 0 and _same_bits(x.cpu().numpy(), x0)
    empty.close(); op.close()


# ---- 7. autograd ------------------------------------------------------------------------------------------------------------------------------

def test_autograd_to_b_coupling_and_S(wlsqm):
    """differentiable_stencil_system_solve through a block solver against the same call through a Jacobi solver: both passes stop at
    rtol, so the two gradients agree within kappa_2(M) rtol times the gradient's norm."""
    import torch
    import wlsqm.hip as whip
    name, points = "elasticity-2D-n130", 8
    sy = BR.system(name)
    n, m = sy["n"], sy["m"]
    s = _system(name)
    kappa = np.linalg.cond(s["M"])
    w = _t(np.random.default_rng(89).standard_normal((n, m)))
    grads = {}
    for pc in ("jacobi", whip.PointBlockJacobi(points)):
        S = _t(sy["S"]).requires_grad_()
        b = _t(sy["b"]).requires_grad_()
        coupling = torch.from_numpy(sy["coupling"].copy()).cuda().requires_grad_()
        op = whip.StencilOperator(sy["dim"], sy["order"], S.detach().clone(), _t(sy["hoods"]), _t(sy["nk"]), _t(sy["knowns"]), _t(sy["wm"]),
                                  _t(sy["rows"]))
        solver = whip.StencilSystemSolver(op, sy["coupling"], diag=sy["diag"], preconditioner=pc)
        x = whip.differentiable_stencil_system_solve(solver, b, S=S, coupling=coupling, rtol=KR.RTOL, maxiter=500)
        (x * w).sum().backward()
        grads[pc if pc == "jacobi" else "blocks"] = [t.grad.cpu().numpy() for t in (b, coupling, S)] + [x.detach().cpu().numpy()]
        solver.close(); op.close()
    for what, gj, gb in zip(("b", "coupling", "S", "x"), grads["jacobi"], grads["blocks"]):
        dist, size = np.linalg.norm(gb - gj), np.linalg.norm(gj)
        print("%s: distance %.3e of norm %.3e, at %.3g of kappa rtol" % (what, dist, size, dist / (kappa * KR.RTOL * size)))
        assert np.isfinite(gb).all() and dist <= kappa * KR.RTOL * size, what


# ---- 8. beside it -----------------------------------------------------------------------------------------------------------------------------

def test_solvers_beside_it_are_not_disturbed(wlsqm):
    import torch
    import wlsqm.hip as whip
    L = wlsqm._binding.lib()
    s = _system("random-m2")
    sy, op = s["sy"], s["op"]
    n = sy["n"]
    rows = SR.rows_of_structure(sy["st"])
    d = 1.0 + 1.5 * 0.75 * np.array([sum(abs(v[0]) for _, v in r) for r in rows])
    rng = np.random.default_rng(73)
    b1, v1 = _t(rng.standard_normal(n)), _t(rng.standard_normal(n))
    scalar = whip.StencilSolver(op, o=0, diag=_t(d), scale=-0.75, preconditioner=whip.BlockJacobi(16))
    jacobi = whip.StencilSystemSolver(op, sy["coupling"], diag=s["diag"])

    def both():
        x = torch.zeros(n, dtype=torch.float64, device="cuda")
        info = scalar.solve(b1, x, maxiter=100)
        after = whip.last_kernel()
        z = scalar.precondition(v1)
        k2 = whip.last_kernel()
        xs = _zeros(n, 2)
        info_s = jacobi.solve(s["b"], xs, maxiter=SR.CAPS["random-m2"]["jacobi"])
        return (info, x, after, k2, z, scalar.memory_used()), (info_s, xs, whip.last_kernel(), jacobi.memory_used())

    ref = both()
    assert ref[0][0].status == ref[1][0].status == 0
    assert ref[0][2:4] == ("krylov-update-block", "krylov-precondition") and ref[1][2] == "krylov-update"
    assert ref[0][5] == L.wlsqm_hip_krylov_workspace_bytes(n) + L.wlsqm_hip_krylov_block_bytes(n, 16)
    assert ref[1][3] == L.wlsqm_hip_krylov_system_workspace_bytes(n, 2)
    blocks = whip.StencilSystemSolver(op, sy["coupling"], diag=s["diag"], preconditioner=whip.PointBlockJacobi(8))
    xb = _zeros(n, 2)
    blocks.enqueue(s["b"], xb, 3)                                        # stopped short
    assert whip.last_kernel() == "krylov-system-update-block" and blocks.info().status == KR.MAXITER
    beside = both()
    info_b = blocks.solve(s["b"], maxiter=BR.CAPS["random-m2", 8, False])
    assert info_b.status == 0
    blocks.precondition(s["b"])
    after = both()
    for got in (beside, after):
        for k in (0, 1):
            assert got[k][0] == ref[k][0] and torch.equal(bits(got[k][1]), bits(ref[k][1])) and got[k][2:4] == ref[k][2:4]
        assert torch.equal(bits(got[0][4]), bits(ref[0][4])) and got[0][5] == ref[0][5]
    scalar.close(); jacobi.close(); blocks.close()
