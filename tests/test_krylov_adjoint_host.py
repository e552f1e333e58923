"""The gradients through implicit solves without a GPU (wlsqm.hip.differentiable_stencil_solve, StencilSolver.gradients, DESIGN.md
section 18): the implicit-gradient formulas of tests/_krylov_adjoint_ref.py against central differences of dense solves, b, diag, scale,
the entries of two rows and the point table along a random unit direction; the transposed systems' iteration counts, to which the GPU
tests' caps are tied; the argument checks on the OnDevice stub (each fails before a kernel is reached); the names in header, binding and
library."""
import os

import numpy as np
import pytest

import _krylov_adjoint_ref as KA
import _krylov_ref as KR
import _stencil_ref as R
from _device_helpers import OnDevice
from test_krylov_host import _operator, _raises

torch = pytest.importorskip("torch")

FIT_SYSTEMS = ("2D-tau0.25-n130", "2D-dirichlet-n130")


@pytest.fixture(scope="module")
def dense():
    """name -> dict(sy, A, d, c, w, grads): the system dense from the oracle's coefficients, the loss L = w . x and its gradients."""
    out = {}
    for name in FIT_SYSTEMS:
        sy = KR.system(name)
        A, d, c = KA.operator_dense(sy), KA.diag_vector(sy), sy["scale"]
        w = KA.adjoint_rhs(sy["n"])
        out[name] = dict(sy=sy, A=A, d=d, c=c, w=w, grads=KA.implicit_gradients(A, d, c, sy["b"], w))
    return out


def _held(formula, fd, what):
    """`fd`: h -> the central difference; the bar at the better of the two steps."""
    rel = [abs(fd(h) - formula) / abs(formula) for h in (1e-5, 1e-6)]
    print("%s: formula %.12e, relative distance %.2e (h = 1e-5), %.2e (h = 1e-6)" % (what, formula, rel[0], rel[1]))
    assert min(rel) <= KA.FD_BAR, (what, formula, rel)


@pytest.mark.parametrize("name", FIT_SYSTEMS)
def test_formulas_against_central_differences(dense, name):
    m = dense[name]
    sy, A, d, c, w, G = m["sy"], m["A"], m["d"], m["c"], m["w"], m["grads"]
    b, n = sy["b"], sy["n"]
    loss = lambda A_, d_, c_, b_: KA.refined_loss(w, np.diag(d_) + c_ * A_, b_)
    rng = np.random.default_rng([53, n])
    unit = lambda *shape: (lambda v: v / np.linalg.norm(v))(rng.standard_normal(shape))
    u = unit(n)
    _held(float(G["b"] @ u), lambda h: KA.central(lambda t: loss(A, d, c, b + t * u), h), name + " b")
    u = unit(n)
    _held(float(G["diag"] @ u), lambda h: KA.central(lambda t: loss(A, d + t * u, c, b), h), name + " diag")
    _held(G["scale"], lambda h: KA.central(lambda t: loss(A, d, c * (1.0 + t), b), h) / c, name + " scale")
    # every entry of two rows: the interior row with the largest |lam|, and the first row of the boundary band (an identity row of the
    # dirichlet system)
    inner = np.flatnonzero(~sy["band"])
    for j in (int(inner[np.argmax(np.abs(G["lam"][inner]))]), int(np.flatnonzero(sy["band"])[0])):
        ks = np.flatnonzero(A[j])
        assert len(ks) >= 1
        worst = 0.0
        for k in ks:
            def moved(t, j=j, k=k):
                A2 = A.copy()
                A2[j, k] += t * abs(A[j, k])
                return loss(A2, d, c, b)
            want = G["entries"][j, k] * abs(A[j, k])
            rel = min(abs(KA.central(moved, h) - want) / abs(want) for h in (1e-5, 1e-6))
            worst = max(worst, rel)
            assert rel <= KA.FD_BAR, (name, j, k, want, rel)
        print("%s row %d: %d entries, worst relative distance %.2e" % (name, j, len(ks), worst))
    # the point table along a random unit direction, the neighbour lists fixed
    T = KA.geometry_truth(sy, G["x"], G["lam"])
    U = unit(*sy["S"].shape)
    _held(float((T * U).sum()), lambda h: KA.central(lambda t: loss(KA.operator_dense(sy, sy["S"] + t * U), d, c, b), h), name + " S")


def test_a_missing_term_shows_at_order_one(dense):
    """What the bar can tell apart: the geometry gradient without its own-point rows, or with lam and x swapped, misses by order 1."""
    m = dense["2D-tau0.25-n130"]
    sy, G = m["sy"], m["grads"]
    T = KA.geometry_truth(sy, G["x"], G["lam"])
    swapped = KA.geometry_truth(sy, G["lam"], G["x"])
    assert np.abs(swapped - T).max() > 1e-2 * np.abs(T).max()


@pytest.mark.parametrize("name", list(KR.SYSTEMS))
def test_transposed_reference_converges_within_the_cap_of_the_gpu_tests(name):
    sy = KR.system(name)
    M = KR.dense_of(sy)
    n = sy["n"]
    g = KA.adjoint_rhs(n)
    x, its, status, hist = KR.bicgstab_ref(M.T, g, np.zeros(n), KR.jacobi(M.T), KR.RTOL, 0.0, 5000)
    print("%s transposed: %d iterations, recorded %d" % (name, its, KA.TRANSPOSED_COUNTS[name]))
    assert status == KR.CONVERGED and hist[-1] <= KR.RTOL * np.linalg.norm(g)
    assert np.array_equal(KR.jacobi(M.T), KR.jacobi(M))                  # the Jacobi diagonal is the same numbers
    if name not in KR.GPU_SYSTEMS:
        return                          # a record only, as the forward solve of this system is
    cap = KA.transposed_maxiter(name)
    assert cap == 2 * KA.TRANSPOSED_COUNTS[name]
    assert 0 < its <= cap <= 3 * its, "set TRANSPOSED_COUNTS[%r] to %d" % (name, its)


def test_statement_and_exact_sum_helpers():
    from fractions import Fraction
    st = KR.square_structure(130, 9, seed=31)
    rows = R.rows_of(st["hoods"], st["nk"], st["slots"], st["own"], st["own_mask"], st["pts"])
    m = R.pack(rows, 1)
    rng = np.random.default_rng(59)
    lam, x = rng.standard_normal(130), rng.standard_normal(130)
    values, diag = KA.grads_statement(m, 130, -0.75, lam, x)
    live = np.zeros(len(values), bool)
    for i, r in enumerate(rows):
        for e, (col, _) in enumerate(r):
            at = m["soff"][i // 64] + 64 * e + i % 64
            live[at] = True
            assert values[at] == -((-0.75 * lam[i]) * x[col])
    assert np.all(values[~live] == 0.0) and not np.signbit(values[~live]).any()
    assert np.array_equal(diag, -(lam * x))
    a, b, c = (rng.standard_normal(40) * 10.0 ** rng.integers(-20, 20, 40) for _ in range(3))
    a[3] = 0.0
    exact, mag = KA.exact_triple(a, b, c)
    terms = [Fraction(float(p)) * Fraction(float(q)) * Fraction(float(r)) for p, q, r in zip(a, b, c)]
    assert exact == sum(terms, Fraction(0)) and mag == sum((abs(t) for t in terms), Fraction(0))
    assert KA.exact_triple([], [], []) == (0, 0)


def test_unpack_and_set_coefficients_on_the_host():
    """unpack is coefficients() for any plane; set_coefficients writes the live entries and leaves the padding; both refuse what
    from_coefficients refuses."""
    import wlsqm.hip as h
    D = OnDevice
    op = _operator(130)
    slots, own = op.coefficients()
    for o in range(op.nop):
        s_o, own_o = op.unpack(D(op._val[o]))
        assert torch.equal(s_o, slots[o]) and torch.equal(own_o, own[o])
    total = op._m["total"]
    _raises("plane must be a contiguous float64 device tensor of shape \\(%d,\\)" % total, op.unpack, D(torch.zeros(total + 1, dtype=torch.float64)))
    _raises("plane must be a contiguous.*strides \\(2,\\)", op.unpack, D(torch.zeros(2 * total, dtype=torch.float64)[::2]))
    _raises("expected 'float64'.*argument plane", op.unpack, D(torch.zeros(total)))
    _raises("argument plane must be a device", op.unpack, torch.zeros(total, dtype=torch.float64))
    _raises("wrong number of dimensions.*argument plane", op.unpack, D(op._val))

    before = op._val.clone()
    pad = torch.ones(total, dtype=torch.bool)
    live, dest, d_own = op._slot_positions()
    pad[dest] = False
    pad[d_own] = False
    new_slots = 2.0 * slots + 1.0
    new_slots[:, ~live] = float("nan")                                   # the padding of the argument may hold anything
    new_own = 3.0 * own - 1.0
    assert op.set_coefficients(D(new_slots), D(new_own)) is op
    got_slots, got_own = op.coefficients()
    assert torch.equal(got_slots[:, live], new_slots[:, live]) and torch.all(got_slots[:, ~live] == 0.0)
    assert torch.equal(got_own[:, op._own_mask], new_own[:, op._own_mask])
    assert torch.equal(op._val[:, pad], before[:, pad]) and op._t is None
    _raises("own goes together with an operator that has own entries", op.set_coefficients, D(new_slots))
    _raises("slots has 1 value planes, the operator 2", op.set_coefficients, D(new_slots[:1]), D(new_own))
    _raises("slots must be at least \\(nop, ncases, 9\\)", op.set_coefficients, D(new_slots[:, :, :8]), D(new_own))
    _raises("own must be at least \\(2, 130\\)", op.set_coefficients, D(new_slots), D(new_own[:, :129]))
    _raises("expected 'float64'.*argument slots", op.set_coefficients, D(new_slots.float()), D(new_own))
    _raises("argument slots must be a device", op.set_coefficients, new_slots, D(new_own))
    op.close()
    _raises("the stencil operator has been closed", op.set_coefficients, D(new_slots), D(new_own))
    _raises("the stencil operator has been closed", op.unpack, D(before[0]))


def test_argument_checks_need_no_device():
    import wlsqm.hip as h
    D = OnDevice
    f64 = torch.float64
    n = 130
    diag = torch.full((n,), 2.0, dtype=f64)
    op = _operator(n)
    solver = h.StencilSolver(op, o=1, diag=D(diag), scale=-0.75)
    total = op._m["total"]
    lam, x, both = torch.zeros(n, dtype=f64), torch.zeros(n, dtype=f64), torch.zeros(2 * n, dtype=f64)
    G = solver.gradients
    _raises("none of values, diag and scale is asked for", G, D(lam), D(x))
    _raises("argument lam must be a device", G, lam, D(x), diag=True)
    _raises("expected 'float64'.*argument x", G, D(lam), D(x.float()), diag=True)
    _raises("lam must be a contiguous float64 device tensor of shape \\(130,\\)", G, D(lam[:-1]), D(x), values=True)
    _raises("lam overlaps x", G, D(both[:n]), D(both[n - 1:2 * n - 1]), scale=True)
    _raises("x overlaps diag", G, D(lam), D(diag), scale=True)
    _raises("lam overlaps workspace", G, D(solver._ws[20:20 + n]), D(x), scale=True)
    _raises("grad_diag must be a contiguous float64 device tensor of shape \\(130,\\)", G, D(lam), D(x), diag=D(both))
    _raises("x overlaps grad_diag", G, D(lam), D(x), diag=D(x))
    _raises("values must be a contiguous float64 device tensor of shape \\(%d,\\)" % total, G, D(lam), D(x), values=D(torch.zeros(total - 1, dtype=f64)))
    _raises("expected 'float64'.*argument values", G, D(lam), D(x), values=D(torch.zeros(total)))
    _raises("argument values must be True, False or a device", G, D(lam), D(x), values=np.zeros(total))
    _raises("values overlaps the operator's values", G, D(lam), D(x), values=D(op._val[1]))
    big = torch.zeros(total + n, dtype=f64)
    _raises("values overlaps lam", G, D(big[total - 1:total - 1 + n]), D(x), values=D(big[:total]))
    _raises("scale must be a float64 device tensor of one element", G, D(lam), D(x), scale=D(torch.zeros(2, dtype=f64)))
    _raises("scale overlaps workspace", G, D(lam), D(x), scale=D(solver._ws[6:7]))

    # transpose=: the same checks, then the transposed matrix is built by the library's own torch operations before the kernels
    b = torch.zeros(n, dtype=f64)
    for call in (solver.solve, lambda b_, x_, **kw: solver.enqueue(b_, x_, 5, **kw)):
        _raises("b overlaps x", call, D(both[:n]), D(both[n - 1:2 * n - 1]), transpose=True)
        _raises("argument b must be a device", call, b, D(x), transpose=True)
        _raises("rtol and atol must be finite and >= 0", call, D(b), D(x), rtol=-1.0, transpose=True)
    assert op._t is None                                                 # nothing was built for a refused call
    _raises("v overlaps out", solver.product, D(both[:n]), out=D(both[1:n + 1]), transpose=True)

    # differentiable_stencil_solve
    F = h.differentiable_stencil_solve
    slots, own = op.coefficients()
    _raises("solver must be a StencilSolver", F, op, D(b))
    _raises("S and coefficients are two ways to make the operator", F, solver, D(b), S=D(torch.zeros(n, 2, dtype=f64)), coefficients=(D(slots), D(own)))
    _raises("coefficients must be \\(slots, own\\)", F, solver, D(b), coefficients=D(slots))
    _raises("coefficients must be \\(slots, own\\)", F, solver, D(b), coefficients=(None, D(own)))
    _raises("made from coefficients: there is no fit to redo", F, solver, D(b), S=D(torch.zeros(n, 2, dtype=f64)))
    _raises("argument b must be a device", F, solver, b)
    _raises("x0 must be a contiguous float64 device tensor of shape \\(130,\\)", F, solver, D(b), x0=D(both))
    _raises("b overlaps x0", F, solver, D(both[:n]), x0=D(both[n - 1:2 * n - 1]))
    _raises("rtol and atol must be finite and >= 0", F, solver, D(b), rtol=float("inf"))
    _raises("rtol and atol must be finite and >= 0", F, solver, D(b), adjoint_rtol=-1e-3)
    _raises("the number of iterations must be", F, solver, D(b), maxiter=-1)
    _raises("check_every must be >= 1", F, solver, D(b), check_every=0)
    op.close()
    _raises("the stencil operator has been closed", G, D(lam), D(x), diag=True)
    _raises("the stencil operator has been closed", F, solver, D(b))
    solver.close()
    _raises("the stencil solver has been closed", G, D(lam), D(x), diag=True)
    _raises("the stencil solver has been closed", F, solver, D(b))


def test_workspace_size_is_unchanged():
    from wlsqm import _binding
    if os.path.exists(_binding.LIB_PATH):
        for n in (1, 130, 257, 65537):
            assert _binding.lib().wlsqm_hip_krylov_workspace_bytes(n) == 8 * (16 + 2 * ((n + 255) // 256) + 9 * n)


def test_header_binding_and_library_name_the_entry_point():
    import subprocess
    from wlsqm import _binding
    import wlsqm.hip as h
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "wlsqm_hip.h")).read()
    binding = open(os.path.join(root, "python-wlsqm_amd", "wlsqm", "_binding.py")).read()
    name = "wlsqm_hip_krylov_grads_device"
    assert " %s(" % name in header and '"krylov-grads"' in header
    assert name in binding
    source = open(os.path.join(root, "python-wlsqm_amd", "csrc", "krylov.hip")).read()
    assert 'note_kernel("krylov-grads")' in source
    if os.path.exists(_binding.LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", _binding.LIB_PATH], capture_output=True, text=True).stdout
        assert " T %s" % name in syms
        assert len(_binding.lib().wlsqm_hip_krylov_grads_device.argtypes) == 18
    assert {"SolveGradients", "differentiable_stencil_solve", "StencilSolver", "StencilOperator"} <= set(h.__all__)
    assert h.SolveGradients(None, 1, 2).diag == 1 and h.SolveGradients._fields == ("values", "diag", "scale")
    for method in ("unpack", "set_coefficients"):
        assert callable(getattr(h.StencilOperator, method))
    assert callable(h.StencilSolver.gradients)
