"""The coupled solves without a GPU (wlsqm.hip.StencilSystemSolver, csrc/krylov.hip): the numpy statements of
tests/_krylov_system_ref.py on every system that tests/test_gpu_krylov_system.py solves — built here from the CPU oracle's
coefficients — converge within the caps that the GPU tests pass, also under the reversed summation order (the admission rule of
sections 21 and 22); the stated order of operations against exact arithmetic; matrix() of a host-built structure against the dense
statement; every refusal and its message on the OnDevice stub; and the names of the entry points."""
import os

import numpy as np
import pytest

import _krylov_ref as KR
import _krylov_system_ref as SR
import _stencil_ref as R
from _device_helpers import OnDevice
from test_krylov_host import _operator, _raises

torch = pytest.importorskip("torch")

CASES = [(name, pc) for name, caps in SR.CAPS.items() for pc in caps]
_dense = {}


def _matrix(name):
    if name not in _dense:
        sy = SR.system(name)
        _dense[name] = (sy, SR.dense_of(sy))
    return _dense[name]


@pytest.fixture(scope="module")
def solved():
    out = {}
    for name, pc in CASES:
        sy, M = _matrix(name)
        b = sy["b"].reshape(-1)
        out[name, pc] = SR.solve_ref(M, b, pc)
        out[name, pc, "reversed"] = SR.solve_ref(M, b, pc, reverse=True)
    return out


@pytest.mark.parametrize("name,pc", CASES)
def test_reference_converges_within_the_cap_of_the_gpu_tests(solved, name, pc):
    sy, M = _matrix(name)
    b = sy["b"].reshape(-1)
    x, its, status, hist = solved[name, pc]
    cap = SR.CAPS[name][pc]
    print("%s %s: %d iterations, maxiter %d" % (name, pc, its, cap))
    assert status == KR.CONVERGED
    assert hist[-1] <= KR.RTOL * np.linalg.norm(b)
    assert np.linalg.norm(b - M @ x) <= 2 * KR.RTOL * np.linalg.norm(b)
    # the cap is twice the count measured here when the constant was set; another BLAS may move the count by a few iterations
    assert 0 < its <= cap, "set the cap of (%r, %r) to %d" % (name, pc, 2 * its)
    assert cap <= 3 * its


@pytest.mark.parametrize("name,pc", CASES)
def test_reversed_summation_order_moves_the_count_by_less_than_a_quarter(solved, name, pc):
    its, status = solved[name, pc][1:3]
    its_r, status_r = solved[name, pc, "reversed"][1:3]
    ratio = max(its, its_r) / min(its, its_r)
    print("%s %s: %d iterations, reversed %d (%.3fx)" % (name, pc, its, its_r, ratio))
    assert status == status_r == KR.CONVERGED
    assert (ratio < 1.25) == ((name, pc) not in SR.HOST_ONLY), "move (%r, %r) %s HOST_ONLY" % (name, pc, "into" if ratio >= 1.25 else "out of")
    assert set(SR.GPU_CASES) == set(CASES) - set(SR.HOST_ONLY)


def test_the_systems_are_what_they_say():
    """The elasticity operator on a quadratic displacement field, whose second derivatives a fit of order 2 reproduces: inside,
    -(mu Lap u + (lambda + mu) grad div u) up to the rounding of the fit; on the band, u itself."""
    for name in ("elasticity-2D-n130", "elasticity-3D-n1000"):
        sy, M = _matrix(name)
        S, dim, n = sy["S"], sy["dim"], sy["n"]
        rng = np.random.default_rng(5)
        H = rng.standard_normal((dim, dim, dim))
        H = H + np.transpose(H, (0, 2, 1))                               # u_a = 1/2 x^T H_a x: d2 u_a / dx_j dx_k = H_a[j, k]
        u = 0.5 * np.einsum("ij,ajk,ik->ia", S, H, S)
        want = np.empty((n, dim))
        for a in range(dim):
            graddiv = sum(H[b][b, a] for b in range(dim))
            want[:, a] = -(SR.MU * np.trace(H[a]) + (SR.LAMBDA + SR.MU) * graddiv)
        want[sy["band"]] = u[sy["band"]]
        got = (M @ u.reshape(-1)).reshape(n, dim)
        assert np.abs(got - want).max() <= 1e-7 * max(1.0, np.abs(want).max()), name
    sy, M = _matrix("reaction-2D-n130")
    assert sy["m"] == 2 and sy["nop"] == 1 and M[0, 1] == sy["diag"][0, 1] == -0.3
    for m in (1, 2, 3, 4):
        sy, M = _matrix("random-m%d" % m)
        assert (sy["m"], sy["nop"]) == (m, SR.RANDOM_NOP[m]) and M.shape == (m * SR.RANDOM_N,) * 2
        d = np.abs(np.diag(M))
        assert np.all(d > np.abs(M).sum(axis=1) - d)                     # strictly diagonally dominant


@pytest.mark.parametrize("m,nop", [(1, 1), (2, 3), (3, 4), (4, 7)])
def test_the_stated_order_against_exact_arithmetic_and_the_dense_matrix(m, nop):
    n = 70
    st = SR.planes_structure(n, 9, nop, seed=7)
    rows = SR.rows_of_structure(st)
    rng = np.random.default_rng([11, m])
    coupling = rng.standard_normal((m, m, nop))
    x = rng.standard_normal((n, m))
    for diag in (0.75, rng.standard_normal((m, m)), rng.standard_normal((m, m, n))):
        y = SR.product_statement(rows, coupling, diag, x)
        exact, mag = SR.exact_product(rows, coupling, diag, x)
        lens = np.array([len(r) for r in rows])
        # per unknown: m nop terms per entry and m of the diagonal block, each sum of n terms within gamma_{n + 1} of its magnitudes
        bound = R.gamma(m * nop * lens + m + 2)[:, None] * mag
        assert np.all(np.abs(y - exact) <= bound)
        M = SR.dense_matrix(SR.dense_planes(rows, n, nop), coupling, diag)
        assert np.all(np.abs((M @ x.reshape(-1)).reshape(n, m) - exact) <= 4 * bound + 1e-300)
        d = SR.jacobi_statement(rows, coupling, diag)
        assert np.all(np.abs(d - np.diag(M)) <= 8 * SR.EPS * (np.abs(SR.diag_blocks(diag, m, n)[range(m), range(m)].T.reshape(-1))
                                                                + np.abs(M).sum(axis=1)))
    assert SR.fma(0.1, 10.0, -1.0) == 2.0 ** -54 and 0.1 * 10.0 - 1.0 == 0.0


def _operator_of(st):
    """A StencilOperator packed from a structure by the library's own torch operations, on host tensors."""
    import wlsqm.hip as h
    op = h.StencilOperator.__new__(h.StencilOperator)
    op._m = op._t = op._tval = op._tpair = None
    t = torch.from_numpy
    op._pack(t(st["hoods"]), t(st["nk"]), t(st["slots"]), t(st["own"]), t(st["own_mask"]), t(st["pts"]).long(), st["npoints"])
    op.known_coef, op.has_known_derivatives, op.no, op._geo, op._rows, op._point_index = None, False, 0, None, None, None
    return op


@pytest.mark.parametrize("m,nop", [(1, 1), (2, 3), (3, 4), (4, 7)])
def test_matrix_of_a_host_built_structure_is_the_dense_statement(m, nop):
    import wlsqm.hip as h
    from wlsqm import _binding
    assert hasattr(h, "StencilSystemSolver")
    if not os.path.exists(_binding.LIB_PATH):
        return                                                           # the constructor asks the library for the workspace's size
    n = 130
    st = SR.planes_structure(n, 9, nop, seed=13)
    rows = SR.rows_of_structure(st)
    A = SR.dense_planes(rows, n, nop)
    rng = np.random.default_rng([17, m])
    coupling = rng.standard_normal((m, m, nop))
    if m > 1:
        coupling[0, 1] = 0.0                                             # a block without a stencil
    tensor = rng.standard_normal((m, m, n))
    for diag in (0.0, 1.5, rng.standard_normal((m, m)), tensor):
        held = OnDevice(torch.from_numpy(diag)) if np.ndim(diag) == 3 else diag
        solver = h.StencilSystemSolver(_operator_of(st), coupling, diag=held)
        if np.ndim(diag) == 3:
            solver.diag = torch.from_numpy(diag)                         # matrix() indexes it: the stub has served the checks
        got = solver.matrix()
        assert got.layout == torch.sparse_csr and tuple(got.shape) == (m * n, m * n)
        want = SR.dense_matrix(A, coupling, diag)
        scale = np.einsum("abo,oij->iajb", np.abs(coupling), np.stack([R.dense([[(c, np.abs(v)) for c, v in r] for r in rows], n, o)
                                                                        for o in range(nop)])).reshape(m * n, m * n)
        assert np.all(np.abs(got.to_dense().numpy() - want) <= 4 * nop * np.finfo(np.float64).eps * scale)
        assert solver.memory_used() == _binding.lib().wlsqm_hip_krylov_system_workspace_bytes(n, m) == 8 * (16 + 2 * ((m * n + 255) // 256) + 9 * m * n)
        solver.close()


def test_refusals_and_argument_checks_need_no_device():
    import wlsqm.hip as h
    D = OnDevice
    f64 = torch.float64
    n = 130
    op = _operator(n)                                                    # two value planes
    cp = np.ones((2, 2, 2))
    S = h.StencilSystemSolver
    _raises("must be a StencilOperator", S, object(), cp)
    _raises("must be square: it has 130 rows \\(cases\\) for 150 points", S, _operator(n, 150), cp)
    _raises("point_index must be None or the identity", S, _operator(n, identity=False, with_pts=True), cp)
    known = _operator(n)
    known.has_known_derivatives = True
    _raises("their affine term belongs in b", S, known, cp)
    closed = _operator(n)
    closed.close()
    _raises("the stencil operator has been closed", S, closed, cp)
    # coupling
    shape = "coupling must have shape \\(m, m, nop\\) with 1 <= m <= 4 and nop = 2, the operator's value planes; got shape "
    _raises(shape + "\\(0, 0, 2\\)", S, op, np.ones((0, 0, 2)))
    _raises(shape + "\\(5, 5, 2\\)", S, op, np.ones((5, 5, 2)))
    _raises(shape + "\\(2, 3, 2\\)", S, op, np.ones((2, 3, 2)))
    _raises(shape + "\\(2, 2, 3\\)", S, op, np.ones((2, 2, 3)))
    _raises(shape + "\\(2, 2\\)", S, op, np.ones((2, 2)))
    for bad in (np.nan, np.inf):
        c = cp.copy()
        c[1, 0, 1] = bad
        _raises("every entry of coupling must be finite", S, op, c)
    # diag
    _raises("diag must be a float, a host array \\(2, 2\\) or a device tensor \\(2, 2, 130\\); got shape \\(3, 3\\)", S, op, cp, diag=np.ones((3, 3)))
    _raises("diag must be a float, a host array", S, op, cp, diag=[1.0, 2.0])
    _raises("every entry of diag must be finite", S, op, cp, diag=float("nan"))
    _raises("diag must be a contiguous float64 device tensor of shape \\(2, 2, 130\\); got shape \\(2, 2, 131\\)", S, op, cp,
            diag=D(torch.ones((2, 2, n + 1), dtype=f64)))
    _raises("diag must be a contiguous float64 device tensor of shape \\(2, 2, 130\\)", S, op, cp, diag=D(torch.ones((n, 2, 2), dtype=f64).permute(1, 2, 0)))
    _raises("wrong number of dimensions.*argument diag", S, op, cp, diag=D(torch.ones((2, n), dtype=f64)))
    _raises("expected 'float64'.*argument diag", S, op, cp, diag=D(torch.ones((2, 2, n))))
    _raises("argument diag must be a device", S, op, cp, diag=torch.ones((2, 2, n), dtype=f64))
    # preconditioner: the two allowed values and nothing else
    for bad in (h.BlockJacobi(16), h.ApproximateInverse(), "ilu", "Jacobi", 1):
        _raises("preconditioner must be 'jacobi' or None", S, op, cp, preconditioner=bad)
    from wlsqm import _binding
    if not os.path.exists(_binding.LIB_PATH):
        return
    diag = torch.ones((2, 2, n), dtype=f64)
    solver = S(op, cp, diag=D(diag), preconditioner=None)
    assert (solver.m, solver.nop, solver.npoints) == (2, 2, n) and solver.refresh() is solver
    b, x = torch.zeros((n, 2), dtype=f64), torch.zeros((n, 2), dtype=f64)
    both = torch.zeros((2 * n + 1, 2), dtype=f64)
    for call in (solver.solve, lambda b_, x_, **kw: solver.enqueue(b_, x_, 5, **kw)):
        _raises("argument b must be a device", call, b, D(x))
        _raises("argument x must be a device", call, D(b), np.zeros((n, 2)))
        _raises("expected 'float64'.*argument b", call, D(b.float()), D(x))
        _raises("wrong number of dimensions.*argument x", call, D(b), D(x[:, 0]))
        _raises("x must be a contiguous float64 device tensor of shape \\(130, 2\\), the m unknowns of a point side by side; got shape "
                "\\(2, 130\\)", call, D(b), D(torch.zeros((2, n), dtype=f64)))
        _raises("b must be a contiguous float64 device tensor of shape \\(130, 2\\).*got shape \\(2, 130\\)", call,
                D(torch.zeros((2, n), dtype=f64)), D(x))
        _raises("b must be a contiguous.*strides \\(1, 130\\)", call, D(torch.zeros((2, n), dtype=f64).t()), D(x))
        _raises("x must be a contiguous.*got shape \\(129, 2\\)", call, D(b), D(x[:-1]))
        _raises("b overlaps x", call, D(both[:n]), D(both[n - 1:2 * n - 1]))
        _raises("x overlaps diag", call, D(b), D(diag.view(-1)[:2 * n].view(n, 2)))
        _raises("b overlaps workspace", call, D(solver._ws[20:20 + 2 * n].view(n, 2)), D(x))
        _raises("rtol and atol must be finite and >= 0", call, D(b), D(x), rtol=-1.0)
    _raises("x must be 16-byte aligned for m = 2", solver.solve, D(b), D(both.view(-1)[1:1 + 2 * n].view(n, 2)))
    _raises("check_every must be >= 1", solver.solve, D(b), D(x), check_every=0)
    _raises("the number of iterations must be", solver.solve, D(b), D(x), maxiter=-1)
    _raises("v overlaps out", solver.product, D(both[:n]), out=D(both[1:n + 1]))
    _raises("w must be a contiguous.*got shape \\(2, 130\\)", solver.product, D(b), D(torch.zeros((2, n), dtype=f64)))
    solver.close()
    solver.close()
    for call in (lambda: solver.solve(D(b), D(x)), lambda: solver.enqueue(D(b), D(x), 3), solver.info, solver.memory_used,
                 lambda: solver.product(D(b)), solver.matrix, solver.refresh):
        _raises("the stencil system solver has been closed", call)


def test_header_binding_and_library_name_the_entry_points():
    import subprocess
    from wlsqm import _binding
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "wlsqm_hip.h")).read()
    binding = open(os.path.join(root, "python-wlsqm_amd", "wlsqm", "_binding.py")).read()
    names = ["wlsqm_hip_krylov_system_workspace_bytes"] + ["wlsqm_hip_krylov_system_%s_device" % s for s in ("start", "bicgstab", "product")]
    for name in names:
        assert " %s(" % name in header
    assert "L.wlsqm_hip_krylov_system_workspace_bytes.argtypes" in binding and '"wlsqm_hip_krylov_system_%s_device"' in binding
    for kernel in ("krylov-system-spmv", "krylov-system-diag"):
        assert '"%s"' % kernel in header
    import wlsqm.hip as h
    assert "StencilSystemSolver" in h.__all__
    if os.path.exists(_binding.LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", _binding.LIB_PATH], capture_output=True, text=True).stdout
        for name in names:
            assert " T %s" % name in syms
        L = _binding.lib()
        assert L.wlsqm_hip_krylov_system_workspace_bytes(-1, 2) == -1 and L.wlsqm_hip_krylov_system_workspace_bytes(130, 5) == -1
        assert L.wlsqm_hip_krylov_system_workspace_bytes(130, 0) == -1
        assert L.wlsqm_hip_krylov_system_workspace_bytes(130, 3) == L.wlsqm_hip_krylov_workspace_bytes(390)
