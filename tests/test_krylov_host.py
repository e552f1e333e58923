"""The implicit solves without a GPU (wlsqm.hip.StencilSolver, csrc/krylov.hip): the numpy statement of the recurrence
(tests/_krylov_ref.py) on every system that tests/test_gpu_krylov.py solves — built here from the CPU oracle's coefficients — converges
within the `maxiter` that the GPU tests pass, so that a cap cannot hide a failure there; its status codes; the argument checks of the
solver on the OnDevice stub (each fails before a kernel is reached); and the names of the entry points in header, binding and library."""
import os

import numpy as np
import pytest

import _krylov_ref as KR
import _stencil_ref as R
from _device_helpers import OnDevice

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def solved():
    """name -> (system, M, x, iterations, status, history) of the reference: Jacobi, zero start, rtol 1e-10, no cap that binds."""
    out = {}
    for name in KR.SYSTEMS:
        sy = KR.system(name)
        M = KR.dense_of(sy)
        out[name] = (sy, M) + KR.bicgstab_ref(M, sy["b"], np.zeros(sy["n"]), KR.jacobi(M), KR.RTOL, 0.0, 5000)
    return out


@pytest.mark.parametrize("name", list(KR.SYSTEMS))
def test_reference_converges_within_the_cap_of_the_gpu_tests(solved, name):
    sy, M, x, its, status, hist = solved[name]
    print("%s: %d iterations, maxiter %d, kappa_2 %.3g" % (name, its, KR.maxiter(name), np.linalg.cond(M)))
    assert status == KR.CONVERGED
    assert len(hist) == its + 1 and hist[-1] <= KR.RTOL * np.linalg.norm(sy["b"])
    if name not in KR.GPU_SYSTEMS:
        return                          # a record only: 383 erratic iterations when measured, a count that any other summation order moves
    # the cap of the GPU tests is twice the count measured here when the constant was set; another BLAS or another compiler's oracle
    # may move the count by a few iterations (more on I - h^2 Lap_h at n = 130, the slowest of them), not by a factor of 1.5
    assert 0 < its <= KR.maxiter(name), "set SYSTEMS[%r]'s maxiter to %d" % (name, 2 * its)
    assert KR.maxiter(name) <= 3 * its


@pytest.mark.parametrize("name", KR.GPU_SYSTEMS)
def test_true_residual_of_the_reference(solved, name):
    """The recursive residual drifts from the true one by the roundings of x += ..., r = s - omega t and of the two products: per
    iteration at most gamma_{L+4} (|M| |x_k| + |r_k|) per component, L the longest row; |x_k| <= ||x||_inf-ish only after the fact, so
    the bound takes 10 times the final iterate's (the iterates of these systems do not overshoot by more)."""
    sy, M, x, its, status, hist = solved[name]
    b = sy["b"]
    true = np.linalg.norm(b - M @ x)
    L = int((M != 0).sum(axis=1).max())
    room = its * 10 * R.gamma(L + 4) * (np.linalg.norm(np.abs(M) @ np.abs(x)) + np.linalg.norm(b))
    print("%s: true %.3e recursive %.3e stop %.3e room %.3e" % (name, true, hist[-1], KR.RTOL * np.linalg.norm(b), room))
    assert true <= KR.RTOL * np.linalg.norm(b) + room
    assert abs(true - hist[-1]) <= room


def test_variants_of_the_first_system_within_their_caps(solved):
    sy, M = solved[KR.FIRST][:2]
    n = sy["n"]
    for what, x0, dinv in (("guess", KR.guess(n), KR.jacobi(M)), ("plain", np.zeros(n), None)):
        x, its, status, hist = KR.bicgstab_ref(M, sy["b"], x0, dinv, KR.RTOL, 0.0, 5000)
        print("%s: %d iterations, maxiter %d" % (what, its, KR.VARIANTS[what]))
        assert status == KR.CONVERGED and np.linalg.norm(sy["b"] - M @ x) <= 2 * KR.RTOL * np.linalg.norm(sy["b"])
        assert 0 < its <= KR.VARIANTS[what] <= 2 * its + 8, "set VARIANTS[%r] to %d" % (what, 2 * its)


def test_exact_dot_in_integers_is_the_fraction_sum():
    rng = np.random.default_rng(47)
    a = rng.standard_normal(300) * 10.0 ** rng.integers(-30, 30, 300)
    b = rng.standard_normal(300) * 10.0 ** rng.integers(-30, 30, 300)
    a[7], b[9] = 0.0, -0.0
    exact, mag = KR.exact_dot(a, b)
    assert exact == R.exact_dot(a, b) and mag == R.exact_dot(np.abs(a), np.abs(b))
    assert KR.exact_dot([], []) == (0, 0)
    st = KR.square_structure(1, 9, seed=1)
    assert len(R.rows_of(st["hoods"], st["nk"], st["slots"], st["own"], st["own_mask"], st["pts"])[0]) == 10
    st = KR.square_structure(130, 9, seed=1)
    assert np.array_equal(st["pts"], np.arange(130)) and st["npoints"] == 130


def test_status_codes_of_the_reference():
    sy = KR.system("random-n130")
    M, b, n = KR.dense_of(sy), sy["b"], sy["n"]
    z = np.zeros(n)
    x, its, status, hist = KR.bicgstab_ref(M, z, z, KR.jacobi(M), 1e-10, 0.0, 100)
    assert (its, status) == (0, KR.CONVERGED) and np.all(x == 0.0)
    M0 = M.copy()
    M0[5, 5] = 0.0
    x0 = np.arange(n, dtype=np.float64)
    x, its, status, hist = KR.bicgstab_ref(M0, b, x0, KR.jacobi(M0), 1e-10, 0.0, 100)
    assert (its, status) == (0, KR.DIAGONAL) and np.array_equal(x, x0)
    bn = b.copy()
    bn[3] = np.nan
    x, its, status, hist = KR.bicgstab_ref(M, bn, z, KR.jacobi(M), 1e-10, 0.0, 100)
    assert (its, status) == (0, KR.NONFINITE) and np.all(x == 0.0)
    x, its, status, hist = KR.bicgstab_ref(M, b, z, KR.jacobi(M), 1e-10, 0.0, 2)
    assert (its, status) == (2, KR.MAXITER) and hist[-1] > 1e-10 * np.linalg.norm(b)
    x, its, status, hist = KR.bicgstab_ref(M, b, z, None, 1e-10, 0.0, 1000)
    assert status == KR.CONVERGED and np.linalg.norm(b - M @ x) <= 1e-9 * np.linalg.norm(b)
    # (t, t) = 0: omega = 0, x += alpha phat, and the ordinary stop test.  M = I answers in one iteration with s = 0.
    x, its, status, hist = KR.bicgstab_ref(np.eye(4), np.arange(1.0, 5.0), np.zeros(4), None, 1e-10, 0.0, 10)
    assert (its, status) == (1, KR.CONVERGED) and np.array_equal(x, np.arange(1.0, 5.0))


def _operator(n=130, npoints=None, identity=True, with_pts=False):
    """A StencilOperator packed from a random structure by the library's own torch operations, on host tensors."""
    import wlsqm.hip as h
    npoints = n if npoints is None else npoints
    st = R.random_structure(n, npoints, 9, 2, seed=3)
    pts = np.arange(n, dtype=np.int32) if identity else st["pts"]
    op = h.StencilOperator.__new__(h.StencilOperator)
    op._m = op._t = op._tval = op._tpair = None
    t = torch.from_numpy
    op._pack(t(st["hoods"]), t(st["nk"]), t(st["slots"]), t(st["own"]), t(st["own_mask"]), t(pts).long(), npoints)
    op.known_coef, op.has_known_derivatives, op.no, op._geo, op._rows = None, False, 0, None, None
    op._point_index = t(pts) if with_pts else None
    return op


class _ReachedTheLibrary(BaseException):
    pass


def _raises(message, fn, *args, **kw):
    """fn raises ValueError / RuntimeError matching `message` before the library is reached."""
    from wlsqm import _binding

    def no_library():
        raise _ReachedTheLibrary()

    real = _binding.lib
    _binding.lib = no_library
    try:
        with pytest.raises((ValueError, RuntimeError), match=message):
            fn(*args, **kw)
    finally:
        _binding.lib = real


def test_argument_checks_need_no_device():
    import wlsqm.hip as h
    D = OnDevice
    f64 = torch.float64
    n = 130
    op = _operator(n)
    _raises("must be a StencilOperator", h.StencilSolver, object())
    _raises("must be square: it has 130 rows \\(cases\\) for 150 points", h.StencilSolver, _operator(n, 150))
    _raises("point_index must be None or the identity", h.StencilSolver, _operator(n, identity=False, with_pts=True))
    known = _operator(n)
    known.has_known_derivatives = True
    _raises("their affine term belongs in b", h.StencilSolver, known)
    closed = _operator(n)
    closed.close()
    _raises("the stencil operator has been closed", h.StencilSolver, closed)
    _raises("the operator has 2 value planes; got o = 2", h.StencilSolver, op, o=2)
    _raises("preconditioner must be 'jacobi' or None", h.StencilSolver, op, preconditioner="ilu")
    _raises("expected 'float64'.*argument diag", h.StencilSolver, op, diag=D(torch.ones(n)))
    _raises("diag must be a contiguous float64 device tensor of shape \\(130,\\)", h.StencilSolver, op, diag=D(torch.ones(n + 1, dtype=f64)))
    _raises("argument diag must be a device", h.StencilSolver, op, diag=torch.ones(n, dtype=f64))

    # the identity as an explicit point_index is accepted; the workspace is what the library says, all of it allocated here
    diag = torch.full((n,), 2.0, dtype=f64)
    solver = h.StencilSolver(_operator(n, with_pts=True), o=1, diag=D(diag), scale=-0.75)
    from wlsqm import _binding
    assert solver.memory_used() == _binding.lib().wlsqm_hip_krylov_workspace_bytes(n) == 8 * (16 + 2 * 1 + 9 * n)
    assert _binding.lib().wlsqm_hip_krylov_workspace_bytes(257) == 8 * (16 + 2 * 2 + 9 * 257)
    b, x = torch.zeros(n, dtype=f64), torch.zeros(n, dtype=f64)
    both = torch.zeros(2 * n, dtype=f64)
    for call in (solver.solve, lambda b_, x_, **kw: solver.enqueue(b_, x_, 5, **kw)):
        _raises("argument b must be a device", call, b, D(x))
        _raises("argument x must be a device", call, D(b), np.zeros(n))
        _raises("expected 'float64'.*argument b", call, D(b.float()), D(x))
        _raises("wrong number of dimensions.*argument x", call, D(b), D(x[None]))
        _raises("x must be a contiguous float64 device tensor of shape \\(130,\\); got shape \\(129,\\)", call, D(b), D(x[:-1]))
        _raises("b must be a contiguous.*strides \\(2,\\)", call, D(both[::2]), D(x))
        _raises("b overlaps x", call, D(both[:n]), D(both[n - 1:2 * n - 1]))
        _raises("x overlaps diag", call, D(b), D(diag))
        _raises("b overlaps workspace", call, D(solver._ws[20:20 + n]), D(x))
        _raises("rtol and atol must be finite and >= 0", call, D(b), D(x), rtol=-1.0)
        _raises("rtol and atol must be finite and >= 0", call, D(b), D(x), atol=float("nan"))
    _raises("check_every must be >= 1", solver.solve, D(b), D(x), check_every=0)
    _raises("the number of iterations must be", solver.solve, D(b), D(x), maxiter=-1)
    _raises("the number of iterations must be", solver.enqueue, D(b), D(x), 2 ** 31)
    _raises("v overlaps out", solver.product, D(both[:n]), out=D(both[1:n + 1]))
    solver._op.close()
    for call in (lambda: solver.solve(D(b), D(x)), lambda: solver.enqueue(D(b), D(x), 3), solver.info, solver.memory_used,
                 lambda: solver.product(D(b))):
        _raises("the stencil operator has been closed", call)
    solver.close()
    solver.close()
    for call in (lambda: solver.solve(D(b), D(x)), lambda: solver.enqueue(D(b), D(x), 3), solver.info, solver.memory_used,
                 lambda: solver.product(D(b))):
        _raises("the stencil solver has been closed", call)


def test_header_binding_and_library_name_the_entry_points():
    import subprocess
    from wlsqm import _binding
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "wlsqm_hip.h")).read()
    binding = open(os.path.join(root, "python-wlsqm_amd", "wlsqm", "_binding.py")).read()
    names = ["wlsqm_hip_krylov_workspace_bytes", "wlsqm_hip_krylov_start_device", "wlsqm_hip_krylov_bicgstab_device",
             "wlsqm_hip_krylov_product_device"]
    for name in names:
        assert " %s(" % name in header
    assert "wlsqm_hip_krylov_workspace_bytes" in binding and 'wlsqm_hip_krylov_%s_device' in binding
    for kernel in ("krylov-spmv-dot", "krylov-update", "krylov-reduce", "krylov-diag"):
        assert '"%s"' % kernel in header
    if os.path.exists(_binding.LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", _binding.LIB_PATH], capture_output=True, text=True).stdout
        for name in names:
            assert " T %s" % name in syms
        L = _binding.lib()
        assert L.wlsqm_hip_krylov_workspace_bytes(-1) == -1
        import wlsqm.hip as h
        assert {"StencilSolver", "SolveInfo"} <= set(h.__all__) and h.SolveInfo(0, 3, 1e-12).iterations == 3
