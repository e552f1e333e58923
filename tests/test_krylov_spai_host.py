"""The sparse approximate inverse preconditioner without a GPU (wlsqm.hip.ApproximateInverse, csrc/krylov.hip):
the two numpy statements of Q (tests/_krylov_spai_ref.py) on every system that tests/test_gpu_krylov_spai.py takes — built here from the
CPU oracle's coefficients; the reference recurrences with that Q converge within the `maxiter` that the GPU tests pass, also under the
reversed summation order (the admission rule of section 21: a count that the order of a sum moves by more than 1.25x is no yardstick);
cond_2 of the Gram matrices and the gap between the two statements, which sets the bar of the GPU comparison; the definition's
properties on hand-made rows; the refusals and argument checks, which need no device; and the names of the entry points."""
import os

import numpy as np
import pytest

import _krylov_ref as KR
import _krylov_spai_ref as SP
from _device_helpers import OnDevice
from test_krylov_host import _operator, _raises

torch = pytest.importorskip("torch")

SOLVED = list(SP.CAPS) + list(SP.HEADLINE)
CASES = [(name, method) for name in SOLVED for method in SP.METHODS]
_dense = {}


def _matrix(name):
    """(system, rows of M, dense M, the reference's rows of Q, dense Q) from the oracle's coefficients, once."""
    if name not in _dense:
        sy = SP.system(name)
        MR = SP.m_rows(SP.rows_of_system(sy), sy["diag"], sy["scale"])
        ref = SP.approximate_inverse_ref(MR)
        _dense[name] = (sy, MR, SP.dense_m(MR), ref, SP.dense_q(ref, sy["n"]))
    return _dense[name]


def _cap(name, method):
    return (SP.HEADLINE[name] if name in SP.HEADLINE else SP.CAPS[name])[method]


@pytest.fixture(scope="module")
def solved():
    out = {}
    for name, method in CASES:
        sy, MR, M, ref, Q = _matrix(name)
        out[name, method] = SP.solve_ref(M, sy["b"], Q, method)
        out[name, method, "reversed"] = SP.solve_ref(M, sy["b"], Q, method, reverse=True)
    return out


def test_the_rows_of_m_are_the_dense_matrix_of_the_other_references():
    for name in ("2D-tau1-n130", "random-n130", "3D-tau1-n130"):
        sy, MR, M, ref, Q = _matrix(name)
        other = KR.dense_of(sy)
        assert np.abs(M - other).max() <= 4 * SP.EPS * np.abs(other).max()       # c * (a + b) against c * a + c * b where a column repeats


@pytest.mark.parametrize("name,method", CASES)
def test_reference_converges_within_the_cap_of_the_gpu_tests(solved, name, method):
    sy, MR, M, ref, Q = _matrix(name)
    x, its, status, hist = solved[name, method]
    cap = _cap(name, method)
    print("%s %s: %d iterations, maxiter %d" % (name, method, its, cap))
    assert status == KR.CONVERGED
    assert hist[-1] <= KR.RTOL * np.linalg.norm(sy["b"])
    assert np.linalg.norm(sy["b"] - M @ x) <= 2 * KR.RTOL * np.linalg.norm(sy["b"])
    # the cap is twice the count measured here when the constant was set; another BLAS may move the count by an iteration or two
    assert 0 < its <= cap, "set the cap of (%r, %r) to %d" % (name, method, 2 * its)
    assert cap <= 3 * its


@pytest.mark.parametrize("name,method", CASES)
def test_reversed_summation_order_moves_the_count_by_less_than_a_quarter(solved, name, method):
    its, status = solved[name, method][1:3]
    its_r, status_r = solved[name, method, "reversed"][1:3]
    ratio = max(its, its_r) / min(its, its_r)
    print("%s %s: %d iterations, reversed %d (%.3fx)" % (name, method, its, its_r, ratio))
    assert status == status_r == KR.CONVERGED
    if name in SP.HEADLINE:
        assert ratio <= 1.25
    else:
        assert (ratio <= 1.25) == ((name, method) not in SP.HOST_ONLY), "move (%r, %r) %s HOST_ONLY" % (name, method, "into" if ratio > 1.25 else "out of")
    assert set(SP.GPU_CASES) == {(n_, m_) for n_, caps in SP.CAPS.items() for m_ in caps} - set(SP.HOST_ONLY)


def test_the_preconditioner_is_what_the_other_ones_are_not(solved):
    """The record that motivates it: I - h^2 Lap_h in 3D at n = 1000 takes BiCGSTAB(2) with blocks of 16 more than ten times the
    iterations (886 when measured)."""
    import _krylov_l2_ref as L2
    name = "3D-tau1-n1000"
    sy, MR, M, ref, Q = _matrix(name)
    x, its, status, hist = L2.solve_ref(M, sy["b"], 16, cap=3000)
    its_q = solved[name, "bicgstab2"][1]
    print("%s: blocks of 16 %d iterations (status %d), the approximate inverse %d" % (name, its, status, its_q))
    assert status == KR.CONVERGED and its >= 10 * its_q


def test_gram_matrices_and_the_gap_between_the_statements():
    """cond_2(G) per row and the gap of the lstsq statement to the Gram statement in the unit eps cond_2(G_i) max |q_i|, over the systems
    of the GPU tests.  The normal equations are accurate enough: the worst cond_2(G) is far from 1 / eps."""
    worst = cond = 0.0
    for name in list(SP.Q_SYSTEMS) + SOLVED:
        sy, MR, M, ref, Q = _matrix(name)
        w = max(SP.gap(r, r["lstsq"]) for r in ref)
        c = max(r["cond"] for r in ref)
        assert all(r["usable"] for r in ref)
        rel = max(np.abs(r["lstsq"] - r["gram"]).max() for r in ref) / np.abs(Q).max()
        print("%s: gap %.3f units, cond_2(G) up to %.3g, |lstsq - Gram| / max |Q| %.3g" % (name, w, c, rel))
        assert rel <= 1e-9
        worst, cond = max(worst, w), max(cond, c)
    print("worst gap %.3f (C0 = %g), worst cond_2(G) %.3g" % (worst, SP.C0, cond))
    assert cond <= 1e9
    assert SP.C0 / 4 <= worst <= SP.C0, "set C0 to %.0f" % np.ceil(1.15 * worst)


def test_transposed_cap():
    name, cap = SP.TRANSPOSED
    sy, MR, M, ref, Q = _matrix(name)
    x, its, status, hist = SP.solve_ref(np.ascontiguousarray(M.T), sy["b"], np.ascontiguousarray(Q.T), "bicgstab2")
    assert status == KR.CONVERGED and 0 < its <= cap <= 3 * its, "set TRANSPOSED's cap to %d" % (2 * its)


def test_the_definition_on_hand_made_rows():
    # a diagonal matrix: Q is its inverse
    MR = [(2.0, []), (4.0, []), (-0.5, [])]
    ref = SP.approximate_inverse_ref(MR)
    assert [r["gram"].tolist() for r in ref] == [[0.5], [0.25], [-2.0]] and all(r["cond"] == 1.0 for r in ref)
    # dead slots: an own entry (column i) and a neighbour named twice take 0.0, and count in the rows of M all the same
    MR = [(1.0, [(1, 0.5), (0, 0.25), (1, 0.125)]), (3.0, [(0, 1.0)])]
    r0 = SP.row_ref(MR, 0)
    assert r0["cols"] == [0, 1, 0, 1] and r0["live"] == [True, True, False, False]
    assert r0["gram"][2] == 0.0 and r0["gram"][3] == 0.0 and r0["lstsq"][2] == 0.0
    M = SP.dense_m(MR)
    assert np.array_equal(M, [[1.25, 0.625], [1.0, 3.0]])
    Q = SP.dense_q(SP.approximate_inverse_ref(MR), 2)
    assert np.allclose(Q, np.linalg.inv(M), rtol=1e-13, atol=0)          # the pattern is full: the least-squares problem is exact
    # invariance under a scaling of the rows of M: q^T D^-1 (D M) is the same problem
    sy, MRs, Ms, ref, Qs = _matrix("2D-dirichlet-n130")
    rng = np.random.default_rng(3)
    s = 10.0 ** rng.uniform(-3, 3, sy["n"])
    scaled = [(d * s[r], [(c, t * s[r]) for c, t in e]) for r, (d, e) in enumerate(MRs)]
    Q2 = SP.dense_q(SP.approximate_inverse_ref(scaled, gram=False), sy["n"])
    assert np.abs(Q2 * s[None, :] - Qs).max() <= 1e-8 * np.abs(Qs).max()
    # a row of zeros: the first pivot is not positive
    q, usable = SP.ldlt_solve(np.zeros((1, 1)), np.zeros(1))
    assert not usable and not q.any()
    q, usable = SP.ldlt_solve(np.array([[1.0, 0.0], [1.0, 1.0]]), np.array([1.0, 1.0]))      # [[1, 1], [1, 1]]: the second pivot is 0
    assert not usable
    q, usable = SP.ldlt_solve(np.array([[4.0, 0.0], [2.0, 5.0]]), np.array([2.0, 3.0]))
    assert usable and np.allclose(np.array([[4.0, 2.0], [2.0, 5.0]]) @ q, [2.0, 3.0], rtol=1e-15)


def test_refusals_and_argument_checks_need_no_device():
    import wlsqm.hip as h
    from wlsqm import _binding
    D = OnDevice
    f64 = torch.float64
    n = 130
    op = _operator(n)
    assert repr(h.ApproximateInverse()) == "ApproximateInverse(refresh=True)" and h.ApproximateInverse(refresh=0).refresh is False
    _raises("an ApproximateInverse preconditions one right-hand side at a time: nfields must be 1; got 3", h.StencilSolver, op,
            preconditioner=h.ApproximateInverse(), nfields=3)
    # the earlier checks keep their order and their words
    _raises("preconditioner must be 'jacobi' or None", h.StencilSolver, op, preconditioner="spai")
    _raises("preconditioner must be 'jacobi' or None", h.StencilSolver, op, preconditioner=h.ApproximateInverse)
    _raises("method must be 'bicgstab' or 'bicgstab2'; got 'gmres'", h.StencilSolver, op, preconditioner=h.ApproximateInverse(), method="gmres")
    _raises("nfields must be an int, 1 .. 8; got 9", h.StencilSolver, op, preconditioner=h.ApproximateInverse(), nfields=9)
    # rows above the cap
    wide = _operator(n)
    wide._nk = wide._nk.clone()
    wide._nk[70] = 65
    _raises("rows of up to 64 neighbours; the operator's longest row has 65", h.StencilSolver, wide, preconditioner=h.ApproximateInverse())
    if not os.path.exists(_binding.LIB_PATH):
        return
    for method, ws in (("bicgstab", _binding.lib().wlsqm_hip_krylov_workspace_bytes(n)), ("bicgstab2", _binding.lib().wlsqm_hip_krylov_l2_workspace_bytes(n))):
        solver = h.StencilSolver(op, preconditioner=h.ApproximateInverse(), method=method)
        total = int(op._m["total"])
        assert solver.memory_used() == ws + _binding.lib().wlsqm_hip_krylov_spai_bytes(n, total) == ws + 8 * (n + 3 + total)
        b, x = torch.zeros(n, dtype=f64), torch.zeros(n, dtype=f64)
        _raises("argument b must be a device", solver.solve, b, D(x))
        _raises("b overlaps the preconditioner's blocks", solver.solve, D(solver._planes[5:5 + n]), D(x))
        _raises("v overlaps out", solver.precondition, D(b), out=D(b))
        _raises("belongs to a BlockJacobi preconditioner", solver.preconditioner_blocks)
        solver.close()
        _raises("the stencil solver has been closed", solver.refresh)
        _raises("the stencil solver has been closed", solver.preconditioner_matrix)
    for other in (h.StencilSolver(op), h.StencilSolver(op, preconditioner=h.BlockJacobi(16))):
        _raises("belongs to an ApproximateInverse preconditioner", other.preconditioner_matrix)
        _raises("belongs to an ApproximateInverse preconditioner", other.preconditioner_coefficients)


def test_header_binding_and_library_name_the_entry_points():
    import subprocess
    from wlsqm import _binding
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "wlsqm_hip.h")).read()
    binding = open(os.path.join(root, "python-wlsqm_amd", "wlsqm", "_binding.py")).read()
    names = ["wlsqm_hip_krylov_spai_bytes"] + ["wlsqm_hip_krylov_spai_%s_device" % s for s in ("build", "apply", "start", "iterate")]
    for name in names:
        assert " %s(" % name in header
    assert "L.wlsqm_hip_krylov_spai_bytes.argtypes" in binding and '"wlsqm_hip_krylov_spai_%s_device"' in binding
    for kernel in ("krylov-spai", "krylov-spai-apply", "krylov-spai-update", "krylov-spai-l2-update"):
        assert '"%s"' % kernel in header
    if os.path.exists(_binding.LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", _binding.LIB_PATH], capture_output=True, text=True).stdout
        for name in names:
            assert " T %s" % name in syms
        L = _binding.lib()
        assert L.wlsqm_hip_krylov_spai_bytes(-1, 0) == -1 and L.wlsqm_hip_krylov_spai_bytes(130, 1000) == 8 * (130 + 3 + 1000)
        import wlsqm.hip as h
        assert "ApproximateInverse" in h.__all__
