"""The gradients through coupled solves without a GPU (wlsqm.hip.differentiable_stencil_system_solve, StencilSystemSolver.gradients,
DESIGN.md section 25): the five formulas of tests/_krylov_system_adjoint_ref.py against central differences of dense solves; the numpy
statement of the gradient kernel against exact arithmetic; the dense statement of M^T; the transposed systems' iteration counts, to
which the GPU tests' caps are tied, and the reversed-order rule for membership of the GPU list; every refusal and its message on the
OnDevice stub; the names in header, binding and library."""
import os

import numpy as np
import pytest

import _krylov_ref as KR
import _krylov_system_adjoint_ref as SA
import _krylov_system_ref as SR
import _stencil_ref as R
from _device_helpers import OnDevice
from test_krylov_host import _operator, _raises

torch = pytest.importorskip("torch")

CASES = [(name, pc) for name, caps in SA.TRANSPOSED_CAPS.items() for pc in caps]


@pytest.fixture(scope="module")
def dense():
    """name -> dict(sy, A, D, w, grads): the system dense from the oracle's coefficients, the loss L = w . x and its gradients."""
    out = {}
    for name in SA.AUTOGRAD_SYSTEMS:
        sy = SR.system(name)
        A = SR.oracle_planes(sy)
        D = SR.diag_blocks(sy["diag"], sy["m"], sy["n"])
        w = SA.adjoint_rhs(sy["n"], sy["m"])
        out[name] = dict(sy=sy, A=A, D=D, w=w, grads=SA.implicit_gradients(A, sy["coupling"], D, sy["b"], w))
    return out


def _held(formula, fd, what):
    """`fd`: h -> the central difference; the bar at the better of the two steps."""
    rel = [abs(fd(h) - formula) / abs(formula) for h in (1e-5, 1e-6)]
    print("%s: formula %.12e, relative distance %.2e (h = 1e-5), %.2e (h = 1e-6)" % (what, formula, rel[0], rel[1]))
    assert min(rel) <= SA.FD_BAR, (what, formula, rel)


@pytest.mark.parametrize("name", SA.AUTOGRAD_SYSTEMS)
def test_formulas_against_central_differences(dense, name):
    """b, diag and coupling along a random unit direction each, the entries of the planes along a random direction on the stored
    pattern; S along a random unit direction on the two fitted systems, the neighbour lists fixed."""
    d = dense[name]
    sy, A, D, w, G = d["sy"], d["A"], d["D"], d["w"], d["grads"]
    b, n, m, cp = sy["b"], sy["n"], sy["m"], sy["coupling"]
    wf = w.reshape(-1)
    loss = lambda A_, cp_, D_, b_: SA.refined_loss(wf, SR.dense_matrix(A_, cp_, D_), b_.reshape(-1))
    rng = np.random.default_rng([71, n, m])
    unit = lambda *shape: (lambda v: v / np.linalg.norm(v))(rng.standard_normal(shape))
    u = unit(n, m)
    _held(float((G["b"] * u).sum()), lambda h: SA.central(lambda t: loss(A, cp, D, b + t * u), h), name + " b")
    u = unit(m, m, n)
    _held(float((G["diag"] * u).sum()), lambda h: SA.central(lambda t: loss(A, cp, D + t * u, b), h), name + " diag")
    u = unit(*cp.shape)
    _held(float((G["coupling"] * u).sum()), lambda h: SA.central(lambda t: loss(A, cp + t * u, D, b), h), name + " coupling")
    # the entries move in proportion to their size, as section 18's test moves them (A + t u is rounded at eps |A|: a step of 1e-6 in
    # absolute terms on second-derivative coefficients of size n would be lost in that rounding), r of unit maximum norm
    r = rng.standard_normal(A.shape)
    u = np.abs(A) * (r / np.abs(r).max())
    _held(float((G["entries"] * u).sum()), lambda h: SA.central(lambda t: loss(A + t * u, cp, D, b), h), name + " entries")
    if sy["kind"] != "random":
        T = SA.geometry_truth(sy, G["x"], G["lam"])
        U = unit(*sy["S"].shape)
        moved = lambda t: loss(SR.oracle_planes(dict(sy, S=sy["S"] + t * U)), cp, D, b)
        _held(float((T * U).sum()), lambda h: SA.central(moved, h), name + " S")


def test_a_missing_term_shows_at_order_one(dense):
    """What the bar can tell apart: (a, b) exchanged in coupling, or lam and x swapped, misses by order 1."""
    d = dense["elasticity-2D-n130"]
    sy, G = d["sy"], d["grads"]
    T = SA.geometry_truth(sy, G["x"], G["lam"])
    assert np.abs(SA.geometry_truth(sy, G["lam"], G["x"]) - T).max() > 1e-2 * np.abs(T).max()
    d = dense["random-m3"]
    G = d["grads"]
    wrong = -np.einsum("ia,oij,jb->bao", G["lam"], d["A"], G["x"])
    assert np.abs(wrong - G["coupling"]).max() > 1e-2 * np.abs(G["coupling"]).max()


@pytest.mark.parametrize("m,nop", [(1, 1), (2, 3), (3, 4), (4, 7)])
def test_the_stated_order_against_exact_arithmetic(m, nop):
    """A value is a sum of m^2 terms c lam x through two fma chains of m roundings each: within gamma_{2 m} of the sum of the terms'
    magnitudes.  The diag is one product.  The padding is no output of the statement: the kernel writes +0.0 there."""
    n = 130
    st = SR.planes_structure(n, 9, nop, seed=7)
    rows = SR.rows_of_structure(st)
    sell = R.pack(rows, nop)
    rng = np.random.default_rng([73, m, nop])
    coupling = rng.standard_normal((m, m, nop))
    lam = rng.standard_normal((n, m)) * 10.0 ** rng.integers(-2, 3, (n, m))
    x = rng.standard_normal((n, m)) * 10.0 ** rng.integers(-2, 3, (n, m))
    at, values, diag = SA.grads_statement(sell, n, coupling, lam, x)
    row, at_all = SA.entries_of(sell, n)
    assert np.array_equal(at, at_all) and values.shape == (nop, len(at))
    exact, mag = SA.exact_values(sell, n, coupling, lam, x)
    assert np.all(np.abs(values - exact) <= float(R.gamma(2 * m)) * mag)
    assert np.array_equal(diag, -np.einsum("ia,ib->abi", lam, x))
    # against the dense formula: entry e of row j in plane o is dL/dA_o[j, col]
    G = -np.einsum("abo,ja,kb->ojk", coupling, lam, x)
    assert np.all(np.abs(values - G[:, row, sell["col"][at]]) <= 4 * float(R.gamma(2 * m)) * mag + 1e-300)
    # the sampled form: the same bits on a subset of the rows
    check = np.array([0, 63, 64, 129])
    at_s, values_s, diag_s = SA.grads_statement(sell, n, coupling, lam, x, check)
    pick = np.isin(row, check)
    assert np.array_equal(at_s, at[pick]) and np.array_equal(values_s, values[:, pick]) and np.array_equal(diag_s, diag[:, :, check])


@pytest.mark.parametrize("m,nop", [(1, 1), (2, 3), (3, 4), (4, 7)])
def test_the_dense_statement_of_the_transposed_system(m, nop):
    n = 70
    st = SR.planes_structure(n, 9, nop, seed=11)
    rows = SR.rows_of_structure(st)
    A = SR.dense_planes(rows, n, nop)
    rng = np.random.default_rng([79, m])
    coupling = rng.standard_normal((m, m, nop))
    for diag in (0.75, rng.standard_normal((m, m)), rng.standard_normal((m, m, n))):
        M = SR.dense_matrix(A, coupling, diag)
        assert np.array_equal(SR.dense_matrix(*SA.transposed_system(A, coupling, diag)), M.T)
        assert np.array_equal(KR.jacobi(M.T), KR.jacobi(M))              # the scalar diagonal is the same numbers
    # the operator packed from the transposed rows has the transposed planes
    hoods, nk, slots = SA.transposed_structure(rows, n, nop)
    trows = R.rows_of(hoods, nk, slots)
    assert np.array_equal(SR.dense_planes(trows, n, nop), np.transpose(A, (0, 2, 1)))


_dense_t = {}


def _transposed(name):
    if name not in _dense_t:
        sy = SR.system(name)
        _dense_t[name] = (sy, np.ascontiguousarray(SR.dense_of(sy).T))
    return _dense_t[name]


@pytest.fixture(scope="module")
def solved():
    out = {}
    for name, pc in CASES:
        sy, Mt = _transposed(name)
        g = SA.adjoint_rhs(sy["n"], sy["m"]).reshape(-1)
        out[name, pc] = SR.solve_ref(Mt, g, pc)
        out[name, pc, "reversed"] = SR.solve_ref(Mt, g, pc, reverse=True)
    return out


@pytest.mark.parametrize("name,pc", CASES)
def test_transposed_reference_converges_within_the_cap_of_the_gpu_tests(solved, name, pc):
    sy, Mt = _transposed(name)
    g = SA.adjoint_rhs(sy["n"], sy["m"]).reshape(-1)
    x, its, status, hist = solved[name, pc]
    cap = SA.TRANSPOSED_CAPS[name][pc]
    print("%s %s transposed: %d iterations, maxiter %d" % (name, pc, its, cap))
    assert status == KR.CONVERGED
    assert hist[-1] <= KR.RTOL * np.linalg.norm(g)
    assert np.linalg.norm(g - Mt @ x) <= 2 * KR.RTOL * np.linalg.norm(g)
    assert 0 < its <= cap, "set the cap of (%r, %r) to %d" % (name, pc, 2 * its)
    assert cap <= 3 * its


@pytest.mark.parametrize("name,pc", CASES)
def test_reversed_summation_order_moves_the_transposed_count_by_less_than_a_quarter(solved, name, pc):
    its, status = solved[name, pc][1:3]
    its_r, status_r = solved[name, pc, "reversed"][1:3]
    ratio = max(its, its_r) / min(its, its_r)
    print("%s %s transposed: %d iterations, reversed %d (%.3fx)" % (name, pc, its, its_r, ratio))
    assert status == status_r == KR.CONVERGED
    assert (ratio < 1.25) == ((name, pc) not in SA.HOST_ONLY), "move (%r, %r) %s HOST_ONLY" % (name, pc, "into" if ratio >= 1.25 else "out of")
    assert set(SA.GPU_CASES) == set(CASES) - set(SA.HOST_ONLY)


def test_refusals_and_argument_checks_need_no_device():
    import wlsqm.hip as h
    from wlsqm import _binding
    if not os.path.exists(_binding.LIB_PATH):
        return                                                           # the constructor asks the library for the workspace's size
    D = OnDevice
    f64 = torch.float64
    n = 130
    op = _operator(n)                                                    # two value planes
    cp = np.arange(8.0).reshape(2, 2, 2)
    diag = torch.ones((2, 2, n), dtype=f64)
    solver = h.StencilSystemSolver(op, cp, diag=D(diag), preconditioner=None)
    total = op._m["total"]
    z = lambda *shape: torch.zeros(shape, dtype=f64)
    lam, x, b, both = z(n, 2), z(n, 2), z(n, 2), z(2 * n + 1, 2)

    # set_coupling: the constructor's checks, and the table replaced
    shape = "coupling must have shape \\(m, m, nop\\) with 1 <= m <= 4 and nop = 2, the operator's value planes; got shape "
    _raises(shape + "\\(2, 2, 3\\)", solver.set_coupling, np.ones((2, 2, 3)))
    _raises(shape + "\\(2, 3, 2\\)", solver.set_coupling, np.ones((2, 3, 2)))
    _raises("the new coupling must keep the solver's shape \\(2, 2, 2\\); got shape \\(3, 3, 2\\)", solver.set_coupling, np.ones((3, 3, 2)))
    _raises("every entry of coupling must be finite", solver.set_coupling, np.full((2, 2, 2), np.nan))
    _raises("coupling must be a host array \\(m, m, nop\\); got a device tensor", solver.set_coupling, D(z(2, 2, 2)))
    assert np.array_equal(solver.coupling, cp) and list(solver._cp) == list(range(8))
    assert solver.set_coupling(2.0 * cp) is solver
    assert np.array_equal(solver.coupling, 2.0 * cp) and list(solver._cp) == [2.0 * v for v in range(8)]
    assert np.array_equal(h.StencilSystemSolver(op, cp, preconditioner=None).coupling, cp)

    # gradients
    G = solver.gradients
    _raises("neither values nor diag is asked for", G, D(lam), D(x))
    _raises("argument lam must be a device", G, lam, D(x), diag=True)
    _raises("expected 'float64'.*argument x", G, D(lam), D(x.float()), diag=True)
    _raises("lam must be a contiguous float64 device tensor of shape \\(130, 2\\)", G, D(lam[:-1]), D(x), values=True)
    _raises("lam overlaps x", G, D(both[:n]), D(both[n - 1:2 * n - 1]), diag=True)
    _raises("x overlaps diag", G, D(lam), D(diag.view(-1)[:2 * n].view(n, 2)), diag=True)
    _raises("lam overlaps workspace", G, D(solver._ws[20:20 + 2 * n].view(n, 2)), D(x), values=True)
    _raises("x must be 16-byte aligned for m = 2", G, D(lam), D(both.view(-1)[1:1 + 2 * n].view(n, 2)), values=True)
    _raises("diag must be a contiguous float64 device tensor of shape \\(2, 2, 130\\), the diag tensor's; got shape \\(2, 2, 131\\)", G,
            D(lam), D(x), diag=D(z(2, 2, n + 1)))
    _raises("diag must be a contiguous.*strides", G, D(lam), D(x), diag=D(z(n, 2, 2).permute(1, 2, 0)))
    room = z(6 * n)
    _raises("grad_diag overlaps x", G, D(lam), D(room[4 * n - 2:6 * n - 2].view(n, 2)), diag=D(room[:4 * n].view(2, 2, n)))
    _raises("grad_diag overlaps diag", G, D(lam), D(x), diag=D(diag))
    _raises("values must be a contiguous float64 device tensor of shape \\(2, %d\\), the operator's layout" % total, G, D(lam), D(x),
            values=D(z(2, total + 1)))
    _raises("wrong number of dimensions.*argument values", G, D(lam), D(x), values=D(z(2 * total)))
    _raises("expected 'float64'.*argument values", G, D(lam), D(x), values=D(torch.zeros((2, total))))
    _raises("argument values must be True, False or a device", G, D(lam), D(x), values=np.zeros((2, total)))
    _raises("values overlaps the operator's values", G, D(lam), D(x), values=D(op._val))
    big = torch.zeros(2 * total + 2 * n, dtype=f64)
    _raises("values overlaps lam", G, D(big[2 * total - 2:2 * total - 2 + 2 * n].view(n, 2)), D(x), values=D(big[:2 * total].view(2, total)))
    _raises("lam overlaps x", solver.coupling_gradient, D(both[:n]), D(both[n - 1:2 * n - 1]))
    _raises("argument x must be a device", solver.coupling_gradient, D(lam), x)

    # transpose=: the same checks; nothing is built for a refused call
    for call in (solver.solve, lambda b_, x_, **kw: solver.enqueue(b_, x_, 5, **kw)):
        _raises("b overlaps x", call, D(both[:n]), D(both[n - 1:2 * n - 1]), transpose=True)
        _raises("argument b must be a device", call, b, D(x), transpose=True)
        _raises("rtol and atol must be finite and >= 0", call, D(b), D(x), rtol=-1.0, transpose=True)
    _raises("v overlaps out", solver.product, D(both[:n]), out=D(both[1:n + 1]), transpose=True)
    assert op._t is None
    assert solver.prepare_transpose() is True and op._t is not None and solver.prepare_transpose() is False
    assert tuple(op._tval.shape) == (2, op._t["total"])                  # all planes

    # differentiable_stencil_system_solve
    F = h.differentiable_stencil_system_solve
    slots, own = op.coefficients()
    _raises("solver must be a StencilSystemSolver", F, h.StencilSolver(op), D(b))
    _raises("S and coefficients are two ways to make the operator", F, solver, D(b), S=D(z(n, 2)), coefficients=(D(slots), D(own)))
    _raises("coefficients must be \\(slots, own\\)", F, solver, D(b), coefficients=D(slots))
    _raises("coefficients must be \\(slots, own\\)", F, solver, D(b), coefficients=(None, D(own)))
    _raises("made from coefficients: there is no fit to redo", F, solver, D(b), S=D(z(n, 2)))
    _raises("coupling must be a float64 torch tensor \\(m, m, nop\\), on the host or on the device", F, solver, D(b), coupling=cp)
    _raises("coupling must be a float64 torch tensor of shape \\(2, 2, 2\\); got torch.float64 of shape \\(2, 2, 3\\)", F, solver, D(b),
            coupling=z(2, 2, 3))
    _raises("coupling must be a float64 torch tensor of shape \\(2, 2, 2\\); got torch.float32", F, solver, D(b), coupling=torch.zeros((2, 2, 2)))
    _raises("argument b must be a device", F, solver, b)
    _raises("x0 must be a contiguous float64 device tensor of shape \\(130, 2\\)", F, solver, D(b), x0=D(both))
    _raises("b overlaps x0", F, solver, D(both[:n]), x0=D(both[n - 1:2 * n - 1]))
    _raises("rtol and atol must be finite and >= 0", F, solver, D(b), rtol=float("inf"))
    _raises("rtol and atol must be finite and >= 0", F, solver, D(b), adjoint_rtol=-1e-3)
    _raises("the number of iterations must be", F, solver, D(b), maxiter=-1)
    _raises("check_every must be >= 1", F, solver, D(b), check_every=0)
    solver.close()
    for call in (lambda: G(D(lam), D(x), diag=True), lambda: F(solver, D(b)), lambda: solver.set_coupling(cp), solver.prepare_transpose,
                 lambda: solver.coupling_gradient(D(lam), D(x)), lambda: solver.solve(D(b), D(x), transpose=True)):
        _raises("the stencil system solver has been closed", call)


def test_header_binding_and_library_name_the_entry_points():
    import subprocess
    from wlsqm import _binding
    import wlsqm.hip as h
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "wlsqm_hip.h")).read()
    binding = open(os.path.join(root, "python-wlsqm_amd", "wlsqm", "_binding.py")).read()
    source = open(os.path.join(root, "python-wlsqm_amd", "csrc", "krylov.hip")).read()
    names = ["wlsqm_hip_krylov_system_%s_transposed_device" % s for s in ("start", "bicgstab", "product")] + ["wlsqm_hip_krylov_system_grads_device"]
    for name in names:
        assert " %s(" % name in header
    assert "wlsqm_hip_krylov_system_grads_device" in binding and '"wlsqm_hip_krylov_system_%s_transposed_device"' in binding
    assert '"krylov-system-grads"' in header and 'note_kernel("krylov-system-grads")' in source
    assert "krylov_system_grads_kernel" in source
    # the existing entry points keep their signatures: the declarations of section 24 stand word for word
    assert ("int wlsqm_hip_krylov_system_product_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width, "
            "const int64_t* soff,\n") in header
    if os.path.exists(_binding.LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", _binding.LIB_PATH], capture_output=True, text=True).stdout
        for name in names:
            assert " T %s" % name in syms
        L = _binding.lib()
        assert len(L.wlsqm_hip_krylov_system_grads_device.argtypes) == 16
        assert L.wlsqm_hip_krylov_system_start_transposed_device.argtypes == L.wlsqm_hip_krylov_system_start_device.argtypes
        for n, m in ((1, 1), (130, 2), (257, 3), (65537, 4)):            # the workspace is what it was
            assert L.wlsqm_hip_krylov_system_workspace_bytes(n, m) == 8 * (16 + 2 * ((m * n + 255) // 256) + 9 * m * n)
    assert {"SystemGradients", "differentiable_stencil_system_solve", "StencilSystemSolver"} <= set(h.__all__)
    assert h.SystemGradients(None, 1).diag == 1 and h.SystemGradients._fields == ("values", "diag")
    for method in ("gradients", "coupling_gradient", "set_coupling", "prepare_transpose"):
        assert callable(getattr(h.StencilSystemSolver, method))
