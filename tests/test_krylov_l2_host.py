"""BiCGSTAB(2) without a GPU (wlsqm.hip.StencilSolver(method="bicgstab2"), csrc/krylov.hip): the numpy statement
of the recurrence (tests/_krylov_l2_ref.py) on every system that tests/test_gpu_krylov_l2.py solves — built here from the CPU oracle's
coefficients — converges within the `maxiter` that the GPU tests pass, also under the reversed summation order; the record that the
method is for (BiCGSTAB with blocks of 16 breaks down on I - h^2 Lap_h in 3D at n = 2000, BiCGSTAB(2) converges); the status codes of the
reference on hand-made systems; the new refusals, which need no device; and the names of the entry points."""
import os

import numpy as np
import pytest

import _krylov_block_ref as KB
import _krylov_l2_ref as L2
import _krylov_ref as KR
import _stencil_ref as R
from test_krylov_host import _operator, _raises

torch = pytest.importorskip("torch")

CASES = ([(name, pc) for name, caps in L2.CAPS.items() for pc in caps] + [(name, 16) for name in L2.HEADLINE])


def _cap(name, pc):
    return L2.HEADLINE[name] if name in L2.HEADLINE else L2.CAPS[name][pc]


_dense = {}


def _matrix(name):
    if name not in _dense:
        sy = L2.system(name)
        _dense[name] = (sy, KR.dense_of(sy))
    return _dense[name]


@pytest.fixture(scope="module")
def solved():
    """(name, precond) -> (x, iterations, status, history) of the reference from zero at rtol 1e-10, no cap that binds; and the same
    under the reversed order at (name, precond, "reversed")."""
    out = {}
    for name, pc in CASES:
        sy, M = _matrix(name)
        out[name, pc] = L2.solve_ref(M, sy["b"], pc)
        out[name, pc, "reversed"] = L2.solve_ref(M, sy["b"], pc, reverse=True)
    return out


@pytest.mark.parametrize("name,pc", CASES)
def test_reference_converges_within_the_cap_of_the_gpu_tests(solved, name, pc):
    sy, M = _matrix(name)
    x, its, status, hist = solved[name, pc]
    cap = _cap(name, pc)
    print("%s %s: %d iterations, maxiter %d" % (name, pc, its, cap))
    assert status == KR.CONVERGED and its % 2 == 0
    assert len(hist) == its // 2 + 1 and hist[-1] <= KR.RTOL * np.linalg.norm(sy["b"])
    # the cap is twice the count measured here when the constant was set; another BLAS may move the count by a cycle or two
    assert 0 < its <= cap, "set the cap of (%r, %r) to %d" % (name, pc, 2 * its)
    assert cap <= 3 * its


@pytest.mark.parametrize("name,pc", CASES)
def test_accuracy_of_the_reference(solved, name, pc):
    """The true residual within the threshold and the drift of the recursive one, bounded as tests/test_krylov_host.py bounds it: per
    iteration 10 gamma_{L+4} (|M| |x| + |b|), L the longest row.  The error within kappa_2(M) times the relative residual (not at
    n = 2000: the GPU test leaves that SVD out too)."""
    sy, M = _matrix(name)
    x, its, status, hist = solved[name, pc]
    b = sy["b"]
    stop, true = KR.RTOL * np.linalg.norm(b), np.linalg.norm(b - M @ x)
    gap = abs(true - hist[-1])
    L = int((M != 0).sum(axis=1).max())
    room = its * 10 * R.gamma(L + 4) * (np.linalg.norm(np.abs(M) @ np.abs(x)) + np.linalg.norm(b))
    print("%s %s: true %.3e recursive %.3e stop %.3e gap %.3e room %.3e" % (name, pc, true, hist[-1], stop, gap, room))
    assert true <= stop + 8 * gap and gap <= room
    if sy["n"] <= 1000:
        xstar = np.linalg.solve(M, b)
        assert np.linalg.norm(x - xstar) / np.linalg.norm(xstar) <= np.linalg.cond(M) * true / np.linalg.norm(b) * (1 + 1e-6)


@pytest.mark.parametrize("name,pc", CASES)
def test_reversed_summation_order_moves_the_count_by_less_than_a_quarter(solved, name, pc):
    """The entry condition of the GPU list: rows and columns reversed, the same blocks.  A pair that leaves 1.25x belongs in HOST_ONLY."""
    its, status = solved[name, pc][1:3]
    its_r, status_r = solved[name, pc, "reversed"][1:3]
    ratio = max(its, its_r) / min(its, its_r)
    print("%s %s: %d iterations, reversed %d (%.3fx)" % (name, pc, its, its_r, ratio))
    assert status == status_r == KR.CONVERGED
    if name in L2.HEADLINE:
        assert ratio <= 1.25
    else:
        assert (ratio <= 1.25) == ((name, pc) not in L2.HOST_ONLY), "move (%r, %r) %s HOST_ONLY" % (name, pc, "into" if ratio > 1.25 else "out of")
    assert set(L2.GPU_CASES) == {(n_, p_) for n_, caps in L2.CAPS.items() for p_ in caps} - set(L2.HOST_ONLY)


def test_bicgstab_breaks_down_where_bicgstab2_converges(solved):
    """The record that motivates the method: I - h^2 Lap_h in 3D, n = 2000, blocks of 16."""
    name = "3D-tau1-n2000"
    sy, M = _matrix(name)
    x, its, status, hist = KB.solve_ref(M, sy["b"], 16, cap=20000)
    x2, its2, status2, hist2 = solved[name, 16]
    print("%s, blocks of 16: BiCGSTAB status %d after %d iterations, BiCGSTAB(2) status %d after %d" % (name, status, its, status2, its2))
    assert status == KR.BREAKDOWN and status2 == KR.CONVERGED
    assert np.linalg.norm(sy["b"] - M @ x2) <= 2 * KR.RTOL * np.linalg.norm(sy["b"])


def test_transposed_cap():
    name, pc, cap = L2.TRANSPOSED
    sy, M = L2.system(name), None
    MT = np.ascontiguousarray(KR.dense_of(sy).T)
    x, its, status, hist = L2.solve_ref(MT, sy["b"], pc)
    assert status == KR.CONVERGED and 0 < its <= cap <= 3 * its, "set TRANSPOSED's cap to %d" % (2 * its)


def test_status_codes_of_the_reference():
    ref = L2.bicgstab2_ref
    z2, e1 = np.zeros(2), np.array([1.0, 0.0])
    X = np.array([[0.0, 1.0], [1.0, 0.0]])
    # the exchange matrix: u1 = X e_1 = e_2, (rt, u1) = 0 with rho0 = 1
    x, its, status, hist = ref(X, e1, z2, None, 1e-10, 0.0, 10)
    assert (its, status) == (0, KR.BREAKDOWN) and np.array_equal(x, z2) and len(hist) == 1
    # b = 0 from x = 0: no division
    assert ref(X, z2, z2, None, 1e-10, 0.0, 10)[1:3] == (0, KR.CONVERGED)
    # a non-finite right-hand side, and x as given
    x0 = np.array([3.0, -1.0])
    x, its, status, hist = ref(X, np.array([np.nan, 1.0]), x0, None, 1e-10, 0.0, 10)
    assert (its, status) == (0, KR.NONFINITE) and np.array_equal(x, x0)
    # a zero on the diagonal under Jacobi, before anything else
    x, its, status, hist = ref(X, e1, x0, KR.jacobi(X), 1e-10, 0.0, 10)
    assert (its, status) == (0, KR.DIAGONAL) and np.array_equal(x, x0)
    # the iteration limit: 0 at once, and an odd limit is passed by one
    T = np.array([[4.0, 1.0, 0.0], [-1.0, 3.0, 1.0], [0.5, 0.0, 5.0]])
    b3 = np.array([1.0, 2.0, 3.0])
    assert ref(T, b3, np.zeros(3), None, 1e-10, 0.0, 0)[1:3] == (0, KR.MAXITER)
    x, its, status, hist = ref(T, b3, np.zeros(3), None, 1e-30, 0.0, 1)
    assert (its, status) == (2, KR.MAXITER) and len(hist) == 2 and hist[1] < hist[0]
    # three rows: the Krylov space is exhausted after two cycles, with every preconditioner
    for pc in (None, "jacobi"):
        x, its, status, hist = ref(T, b3, np.zeros(3), L2.preconditioner(T, pc), 1e-10, 0.0, 10)
        assert (its, status) == (4, KR.CONVERGED) and np.allclose(T @ x, b3, rtol=0, atol=1e-9)
    # M = I: r vanishes in the step j = 0, so (rt, u2) = 0: the breakdown waits, s1 = 0 takes g1 = g2 = 0, x receives alpha_0 u_0 = b
    x, its, status, hist = ref(np.eye(2), np.array([1.0, 2.0]), z2, None, 1e-10, 0.0, 10)
    assert (its, status) == (2, KR.CONVERGED) and np.array_equal(x, [1.0, 2.0]) and hist[-1] == 0.0
    # ... and at rtol = 0 the same cycle converges on (r, r) = 0, before the next one could answer 2 for omega = 0
    assert ref(np.eye(2), np.array([1.0, 2.0]), z2, None, 0.0, 0.0, 10)[1:3] == (2, KR.CONVERGED)
    # one row: the Krylov space has one dimension, so every solve meets (rt, u2) = 0 in its first cycle, and converges in it
    rng = np.random.default_rng(5)
    for _ in range(200):
        m1, b1 = np.array([[rng.standard_normal() + 3.0]]), rng.standard_normal(1)
        for pc in (None, "jacobi"):
            x, its, status, hist = ref(m1, b1, np.zeros(1), L2.preconditioner(m1, pc), 1e-10, 0.0, 50)
            assert (its, status) == (2, KR.CONVERGED) and abs(m1[0, 0] * x[0] - b1[0]) <= 1e-10 * abs(b1[0])
    # the minimisation's two rules
    assert L2.minimise(0.0, 0.0, 0.0, 0.0, 0.0) == (0.0, 0.0)
    assert L2.minimise(4.0, 2.0, 8.0, 16.0, 4.0) == (0.5, 0.0)            # r2 = 2 r1: s2 = 16 - 2 * 8 = 0
    g1, g2 = L2.minimise(1.0, 1.0, 0.0, 4.0, 2.0)                        # r1 and r2 orthogonal
    assert (g1, g2) == (1.0, 0.5)


def test_argument_refusals_need_no_device():
    import wlsqm.hip as h
    op = _operator(130)
    _raises("method must be 'bicgstab' or 'bicgstab2'; got 'gmres'", h.StencilSolver, op, method="gmres")
    _raises("method must be 'bicgstab' or 'bicgstab2'; got None", h.StencilSolver, op, method=None)
    _raises("method 'bicgstab2' solves one right-hand side at a time: nfields must be 1; got 2", h.StencilSolver, op, method="bicgstab2", nfields=2)
    # the earlier checks keep their order and their words
    _raises("nfields must be an int, 1 .. 8; got 9", h.StencilSolver, op, method="gmres", nfields=9)
    _raises("preconditioner must be 'jacobi' or None", h.StencilSolver, op, preconditioner="ilu", method="bicgstab2")


def test_header_binding_and_library_name_the_entry_points():
    import subprocess
    from wlsqm import _binding
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "wlsqm_hip.h")).read()
    binding = open(os.path.join(root, "python-wlsqm_amd", "wlsqm", "_binding.py")).read()
    names = ["wlsqm_hip_krylov_l2_workspace_bytes", "wlsqm_hip_krylov_l2_start_device", "wlsqm_hip_krylov_l2_device"]
    for name in names:
        assert " %s(" % name in header and "L.%s.argtypes" % name in binding
    for kernel in ("krylov-l2-update", "krylov-l2-update-block", "krylov-l2-reduce"):
        assert '"%s"' % kernel in header
    if os.path.exists(_binding.LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", _binding.LIB_PATH], capture_output=True, text=True).stdout
        for name in names:
            assert " T %s" % name in syms
        L = _binding.lib()
        assert L.wlsqm_hip_krylov_l2_workspace_bytes(-1) == -1
        assert L.wlsqm_hip_krylov_l2_workspace_bytes(257) == 8 * (16 + 5 * 2 + 10 * 257)
        import inspect
        import wlsqm.hip as h
        assert inspect.signature(h.StencilSolver.__init__).parameters["method"].default == "bicgstab"
