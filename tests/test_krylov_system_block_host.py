"""The block-Jacobi preconditioner over points without a GPU (wlsqm.hip.PointBlockJacobi, csrc/krylov.hip): the
stated entries of the blocks against exact arithmetic and the dense M; the elimination's statement on the padded blocks against an
mpmath solve (STATEMENT_RATIO); the layout's row mapping; the iteration counts of tests/_krylov_system_block_ref.bicgstab on every
(system, points) pair that tests/test_gpu_krylov_system_block.py solves — from the CPU oracle's coefficients — within the caps, also
under the reversed summation order; the gain over the scalar diagonal; every refusal and its message on the OnDevice stub; the C
side's WLSQM_EVALUE returns; and the names of the entry points."""
import ctypes as C
import os

import numpy as np
import pytest

import _krylov_block_ref as KB
import _krylov_ref as KR
import _krylov_system_block_ref as BR
import _krylov_system_ref as SR
import _stencil_ref as R
from _device_helpers import OnDevice
from test_krylov_host import _operator, _raises

torch = pytest.importorskip("torch")

CASES = list(BR.CAPS)
_dense = {}


def _matrix(key):
    if key not in _dense:
        _dense[key] = BR.matrix_of(key)
    return _dense[key]


@pytest.fixture(scope="module")
def solved():
    out = {}
    for key in CASES:
        sy, M, b = _matrix(key)
        out[key] = BR.solve_ref(M, b, sy["m"], key[1])
        out[key, "reversed"] = BR.solve_ref(M, b, sy["m"], key[1], reverse=True)
    return out


@pytest.mark.parametrize("key", CASES, ids=lambda k: "%s-%d%s" % (k[0], k[1], "-T" if k[2] else ""))
def test_reference_converges_within_the_cap_of_the_gpu_tests(solved, key):
    sy, M, b = _matrix(key)
    x, its, status, hist = solved[key]
    cap = BR.CAPS[key]
    print("%s: %d iterations, maxiter %d" % (key, its, cap))
    assert status == KR.CONVERGED
    assert hist[-1] <= KR.RTOL * np.linalg.norm(b)
    assert np.linalg.norm(b - M @ x) <= 2 * KR.RTOL * np.linalg.norm(b)
    # the cap is twice the count measured here when the constant was set; another BLAS may move the count by a few iterations
    assert 0 < its <= cap, "set the cap of %r to %d" % (key, 2 * its)
    assert cap <= 3 * its


@pytest.mark.parametrize("key", CASES, ids=lambda k: "%s-%d%s" % (k[0], k[1], "-T" if k[2] else ""))
def test_reversed_summation_order_moves_the_count_by_less_than_a_quarter(solved, key):
    its, status = solved[key][1:3]
    its_r, status_r = solved[key, "reversed"][1:3]
    ratio = max(its, its_r) / min(its, its_r)
    print("%s: %d iterations, reversed %d (%.3fx)" % (key, its, its_r, ratio))
    assert status == status_r == KR.CONVERGED
    assert (ratio < 1.25) == (key not in BR.HOST_ONLY), "move %r %s HOST_ONLY" % (key, "into" if ratio >= 1.25 else "out of")
    assert set(BR.GPU_CASES) == set(CASES) - set(BR.HOST_ONLY)
    assert 4 * len(BR.GPU_CASES) >= 3 * len(CASES)                        # the GPU list keeps three quarters of the pairs


@pytest.mark.parametrize("name,points", BR.GAIN)
def test_the_gain_over_the_scalar_diagonal(solved, name, points):
    """The ratio of the blocks' count to Jacobi's, both by the reference on the oracle's coefficients: the rehearsal measured 96 / 213
    on 2D elasticity at 1000 points with 8 points per block; another BLAS moves either count by the reversed-order margin at most."""
    sy, M, b = _matrix((name, points, False))
    its = solved[name, points, False][1]
    jac = SR.solve_ref(M, b, "jacobi")
    assert jac[2] == KR.CONVERGED
    ratio = its / jac[1]
    print("%s with %d points: %d iterations against Jacobi's %d, ratio %.3f" % (name, points, its, jac[1], ratio))
    assert ratio == BR.gain_ratio(M, b, sy["m"], points)
    assert (96 / 213) / 1.25 <= ratio <= (96 / 213) * 1.25


@pytest.mark.parametrize("m,nop", [(1, 1), (2, 3), (3, 4), (4, 7)])
def test_the_stated_entries_against_exact_arithmetic_and_the_dense_matrix(m, nop):
    n = 70
    st = SR.planes_structure(n, 9, nop, seed=7)
    rows = SR.rows_of_structure(st)
    A = SR.dense_planes(rows, n, nop)
    rng = np.random.default_rng([11, m])
    lens = np.array([len(r) for r in rows])
    for points in {1: (8, 32), 2: (1, 7, 16), 3: (2, 5, 10), 4: (3, 8)}[m]:
        for coupling in (rng.standard_normal((m, m, nop)), rng.standard_normal((m, m, nop, n))):
            for diag in (0.75, rng.standard_normal((m, m)), rng.standard_normal((m, m, n))):
                got = BR.block_statement(rows, coupling, diag, points)
                exact, mag = BR.exact_blocks(rows, coupling, diag, points)
                rows_of_block = m * points
                nblocks = (n + points - 1) // points
                assert got.shape == exact.shape == (nblocks, rows_of_block, rows_of_block)
                # an entry: at most nop terms per duplicate of its column and one of D, each sum within gamma of its magnitudes
                point_of = np.minimum((np.arange(nblocks)[:, None] * points + np.arange(rows_of_block)[None, :] // m), n - 1)
                bound = R.gamma(nop * lens[point_of] + 2)[:, :, None] * mag
                assert np.all(np.abs(got - exact) <= bound)
                dense = BR.point_blocks_of(BR.dense_matrix(A, coupling, diag), m, points)
                assert np.all(np.abs(dense - exact) <= 4 * bound + 1e-300)
                cut = n - (nblocks - 1) * points
                if cut < points:                                         # what the cut last block leaves over is the exact identity
                    rest = got[-1].copy()
                    rest[:cut * m, :cut * m] = np.eye(cut * m)
                    assert np.array_equal(rest, np.eye(rows_of_block))


def test_the_layout_maps_every_row_once_and_sizes_the_plane():
    from wlsqm import _binding
    for m, pts in BR.BLOCK_POINTS.items():
        assert BR.default_points(m) == {1: 16, 2: 8, 3: 5, 4: 4}[m]
        for points in pts:
            for n in BR.BLOCK_SIZES + (1000,):
                lay = BR.layout(n, m, points)
                live = lay["row"][lay["row"] >= 0]
                assert np.array_equal(live, np.arange(m * n))            # every flat row once, in order
                assert lay["nb"] == BR.nb_of(m * points) >= m * points and lay["per"] * lay["nb"] == 64
                assert lay["nwaves"] * lay["per"] >= lay["nblocks"] == -(-n // points)
                if os.path.exists(_binding.LIB_PATH):
                    L = _binding.lib()
                    assert L.wlsqm_hip_krylov_system_block_bytes(n, m, points) == 8 * lay["doubles"]
                    if m * points == lay["nb"]:                          # R = NB: section 19's plane at m n rows
                        assert 8 * lay["doubles"] == L.wlsqm_hip_krylov_block_bytes(m * n, lay["nb"])
    # blocks_of_plane inverts the layout
    n, m, points = 17, 3, 5
    lay = BR.layout(n, m, points)
    nb, per, nwaves = lay["nb"], lay["per"], lay["nwaves"]
    blocks = np.random.default_rng(3).standard_normal((nwaves * per, nb, nb))
    plane = np.zeros(lay["doubles"])
    for w in range(nwaves):
        for lane in range(64):
            for j in range(nb):
                plane[(w * nb + j) * 64 + lane] = blocks[w * per + lane // nb, lane % nb, j]
    assert np.array_equal(BR.blocks_of_plane(plane, n, m, points), blocks)


def _ratio_of(blocks):
    nb = blocks.shape[1]
    inv = np.stack([KB.gauss_jordan_statement(B)[0] for B in blocks])
    v = np.random.default_rng(5).standard_normal(blocks.shape[0] * nb)
    return KB.worst_ratio(blocks, KB.apply_blocks(inv, v), KB.mp_block_solve(blocks, v), nb)


def test_the_elimination_statement_on_the_padded_blocks_against_mpmath():
    pytest.importorskip("mpmath")
    worst = 0.0
    for name, points in BR.STATEMENT_ON:
        sy, M, b = _matrix((name, points, False))
        worst = max(worst, _ratio_of(BR.pad_blocks(BR.point_blocks_of(M, sy["m"], points))))
    for m, n, points, form, point in BR.block_cases():
        st, rows, coupling, diag = BR.block_case(n, m, form, point)
        worst = max(worst, _ratio_of(BR.pad_blocks(BR.block_statement(rows, coupling, diag, points))))
    print("the statement's worst ratio: %.4f (STATEMENT_RATIO %.4f)" % (worst, BR.STATEMENT_RATIO))
    assert worst <= BR.STATEMENT_RATIO <= 2 * worst


def test_the_singular_point_block_sits_in_a_regular_matrix():
    sy = BR.singular_point_system()
    rows = SR.rows_of_structure(sy["st"])
    M = SR.dense_matrix(SR.dense_planes(rows, sy["n"], 1), sy["coupling"], sy["diag"])
    assert np.array_equal(M[:2, :2], np.ones((2, 2))) and np.all(np.diag(M) != 0.0)
    assert np.linalg.cond(M) < 1e3
    b = sy["b"].reshape(-1)
    x, its, status, hist = SR.solve_ref(M, b, "jacobi")
    assert status == KR.CONVERGED and its <= 2 * len(b)                         # Jacobi's reference goes through
    assert not KB.gauss_jordan_statement(BR.pad_blocks(BR.point_blocks_of(M, 2, 1))[0])[1]
    assert all(KB.gauss_jordan_statement(B)[1] for B in BR.pad_blocks(BR.point_blocks_of(M, 2, 1))[1:])


def test_refusals_and_argument_checks_need_no_device():
    import wlsqm.hip as h
    D = OnDevice
    f64 = torch.float64
    n = 130
    op = _operator(n)                                                    # two value planes
    cp = np.ones((2, 2, 2))
    S, P = h.StencilSystemSolver, h.PointBlockJacobi
    assert "PointBlockJacobi" in h.__all__
    assert repr(P()) == "PointBlockJacobi(points=None, refresh=True)" and repr(P(3, refresh=0)) == "PointBlockJacobi(points=3, refresh=False)"
    for bad in (0, -1, 2.0, "8", True, (4,)):
        with pytest.raises(ValueError, match="points must be None or an int >= 1, the points of a block; got"):
            P(bad)
    _raises("points must be 1 .. 16 for m = 2: a block holds m points <= 32 rows; got 17", S, op, cp, preconditioner=P(17))
    _raises("points must be 1 .. 10 for m = 3: a block holds m points <= 32 rows; got 11", S, op, np.ones((3, 3, 2)), preconditioner=P(11))
    _raises("points must be 1 .. 32 for m = 1: a block holds m points <= 32 rows; got 33", S, op, np.ones((1, 1, 2)), preconditioner=P(33))
    _raises("points must be 1 .. 8 for m = 4", S, op, D(torch.zeros((4, 4, 2, n), dtype=f64)), preconditioner=P(9))
    _raises("a PointBlockJacobi belongs to a StencilSystemSolver, whose blocks count points of m unknowns; a StencilSolver takes a "
            "BlockJacobi, whose block counts rows", h.StencilSolver, op, preconditioner=P(8))
    for bad in (h.BlockJacobi(16), h.ApproximateInverse(), "ilu", P):
        _raises("preconditioner must be 'jacobi' or None, or a PointBlockJacobi, for coupled fields", S, op, cp, preconditioner=bad)
    # the earlier checks keep their order and their words
    _raises("must be a StencilOperator", S, object(), cp, preconditioner=P(99))
    _raises("coupling must have shape", S, op, np.ones((2, 3, 2)), preconditioner=P(99))
    from wlsqm import _binding
    if not os.path.exists(_binding.LIB_PATH):
        return
    L = _binding.lib()
    for m, want in ((1, 16), (2, 8), (3, 5), (4, 4)):
        solver = S(op, np.ones((m, m, 2)), preconditioner=P())
        assert (solver.block_points, solver.block_rows) == (want, m * want)
        assert solver.memory_used() == L.wlsqm_hip_krylov_system_workspace_bytes(n, m) + L.wlsqm_hip_krylov_system_block_bytes(n, m, want)
        solver.close()
    jac = S(op, cp)
    assert (jac.block_points, jac.block_rows) == (None, None)
    _raises("precondition\\(\\) belongs to a PointBlockJacobi preconditioner", jac.precondition, D(torch.zeros((n, 2), dtype=f64)))
    _raises("preconditioner_blocks\\(\\) belongs to a PointBlockJacobi preconditioner", jac.preconditioner_blocks)
    solver = S(op, cp, preconditioner=P(3))
    assert (solver.block_points, solver.block_rows) == (3, 6)
    b, x = torch.zeros((n, 2), dtype=f64), torch.zeros((n, 2), dtype=f64)
    plane = solver._planes[:2 * n].view(n, 2)
    _raises("b overlaps the preconditioner's blocks", solver.solve, D(plane), D(x))
    _raises("v must be a contiguous float64 device tensor of shape \\(130, 2\\)", solver.precondition, D(torch.zeros((2, n), dtype=f64)))
    _raises("v overlaps out", solver.precondition, D(b), out=D(b))
    solver.close()
    for call in (solver.refresh, solver.preconditioner_blocks, lambda: solver.precondition(D(b))):
        _raises("the stencil system solver has been closed", call)


def test_the_c_side_refuses_before_any_launch():
    from wlsqm import _binding
    if not os.path.exists(_binding.LIB_PATH):
        return
    L = _binding.lib()
    assert L.wlsqm_hip_krylov_system_block_bytes(130, 2, 17) == -1 and L.wlsqm_hip_krylov_system_block_bytes(130, 5, 1) == -1
    assert L.wlsqm_hip_krylov_system_block_bytes(130, 3, 0) == -1 and L.wlsqm_hip_krylov_system_block_bytes(-1, 2, 8) == -1
    assert L.wlsqm_hip_krylov_system_block_bytes(0, 2, 8) == 0
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)                                          # 16-byte aligned host memory: no launch is reached
    assert p.value % 16 == 0
    odd = C.c_void_p(p.value + 8)
    coupled = lambda m: (130, 3, p, p, p, p, p, 100, 2, m, p, None, p)
    point = lambda m: coupled(m) + (0, None)
    start, iterate = (p, p, 1e-10, 0.0, 10, p, 0, None), (p, 5, p, 0, None)
    last = lambda: L.wlsqm_hip_last_error().decode()
    calls = []
    for tr in ("", "_transposed"):
        calls.append((getattr(L, "wlsqm_hip_krylov_system_block_start%s_device" % tr), coupled, start, "krylov_system_block_start" + tr))
        calls.append((getattr(L, "wlsqm_hip_krylov_system_block_bicgstab%s_device" % tr), coupled, iterate, "krylov_system_block_bicgstab" + tr))
    calls.append((L.wlsqm_hip_krylov_system_point_block_start_device, point, start, "krylov_system_point_block_start"))
    calls.append((L.wlsqm_hip_krylov_system_point_block_bicgstab_device, point, iterate, "krylov_system_point_block_bicgstab"))
    calls.append((L.wlsqm_hip_krylov_system_block_factor_device, lambda m: coupled(m) + (0,), "factor", "krylov_system_block_factor"))
    calls.append((L.wlsqm_hip_krylov_system_block_gather_device, lambda m: coupled(m) + (0,), "gather", "krylov_system_block_gather"))
    for fn, head, tail, who in calls:
        if tail == "factor":
            rest = lambda planes: (planes, None, 0, None)
        elif tail == "gather":
            rest = lambda planes: (planes, 0, None)
        else:
            rest = lambda planes, tail=tail: (planes,) + tail
        assert fn(*head(2), 17, *rest(p)) == _binding.WLSQM_EVALUE
        assert last() == who + ": points must be 1 .. 16 for m = 2 (m points <= 32)"
        assert fn(*head(3), 11, *rest(p)) == _binding.WLSQM_EVALUE and "points must be 1 .. 10 for m = 3" in last()
        assert fn(*head(2), 0, *rest(p)) == _binding.WLSQM_EVALUE and "points must be 1 .. 16" in last()
        assert fn(*head(5), 1, *rest(p)) == _binding.WLSQM_EVALUE and last() == who + ": m must be 1 .. 4"
        assert fn(*head(2), 8, *rest(None)) == _binding.WLSQM_EVALUE and last() == who + ": null array"
        assert fn(*head(2), 8, *rest(odd)) == _binding.WLSQM_EVALUE
        assert last() == who + ": with m = 2 or 4 the block planes must be 16-byte aligned"
    fn = L.wlsqm_hip_krylov_system_block_precondition_device
    who = "krylov_system_block_precondition"
    assert fn(130, 2, 17, p, p, p, 0, None) == _binding.WLSQM_EVALUE and "points must be 1 .. 16 for m = 2" in last()
    assert fn(130, 2, 8, None, p, p, 0, None) == _binding.WLSQM_EVALUE and last() == who + ": null array"
    assert fn(130, 2, 8, odd, p, p, 0, None) == _binding.WLSQM_EVALUE and "16-byte aligned" in last()
    assert fn(130, 2, 8, p, None, p, 0, None) == _binding.WLSQM_EVALUE and last() == who + ": null array"
    assert fn(0, 2, 8, p, p, p, 0, None) == _binding.WLSQM_EVALUE and "npoints must be >= 1" in last()
    # the factor's own checks, still ahead of the device
    fn = L.wlsqm_hip_krylov_system_block_factor_device
    assert fn(130, 2, p, p, p, p, p, 100, 2, 2, p, None, p, 0, 8, p, None, 0, None) == _binding.WLSQM_EVALUE
    assert "npoints must be 1 .. 64 \\* nslices".replace("\\", "") in last()
    assert fn(130, 3, p, p, p, p, p, 100, 9, 2, p, None, p, 0, 8, p, None, 0, None) == _binding.WLSQM_EVALUE and "nop must be 1 .. 8" in last()
    assert fn(130, 3, p, p, p, p, p, 100, 2, 2, None, None, p, 0, 8, p, None, 0, None) == _binding.WLSQM_EVALUE and "null array" in last()
    assert fn(130, 3, p, p, p, p, p, 100, 2, 2, p, None, p, 0, 8, p, odd, 0, None) == _binding.WLSQM_EVALUE and "16-byte aligned" in last()


def test_header_binding_and_library_name_the_entry_points():
    import subprocess
    from wlsqm import _binding
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "wlsqm_hip.h")).read()
    binding = open(os.path.join(root, "python-wlsqm_amd", "wlsqm", "_binding.py")).read()
    names = ["wlsqm_hip_krylov_system_block_bytes"] + ["wlsqm_hip_krylov_system_%s_device" % s for s in (
        "block_factor", "block_gather", "block_precondition", "block_start", "block_bicgstab", "block_start_transposed", "block_bicgstab_transposed",
        "point_block_start", "point_block_bicgstab")]
    for name in names:
        assert " %s(" % name in header
    assert "L.wlsqm_hip_krylov_system_block_bytes.argtypes" in binding and 'hasattr(L, "wlsqm_hip_krylov_system_block_factor_device")' in binding
    for kernel in ("krylov-system-blocks", "krylov-system-update-block", "krylov-system-precondition"):
        assert '"%s"' % kernel in header
    record = open(os.path.join(root, "profiles", "isa_krylov_system_block.txt")).read().splitlines()
    kernels = [line for line in record if line.startswith("krylov_system_")]
    assert len(kernels) == 12 and all("scratch     0 B" in line and "spilled    0" in line for line in kernels)
    if os.path.exists(_binding.LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", _binding.LIB_PATH], capture_output=True, text=True).stdout
        for name in names:
            assert " T %s" % name in syms
