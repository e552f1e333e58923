"""Coupled solves with a per-point coupling without a GPU (wlsqm.hip.StencilSystemSolver with a device tensor (m, m, nop, npoints),
csrc/krylov.hip): the stated orders of operations of tests/_krylov_system_point_ref.py against exact rational
arithmetic and the per-point dense matrix; matrix() of a host-built structure against that dense statement; a table that is constant
over the points against _krylov_system_ref.dense_matrix, exactly; the iteration counts behind the GPU tests' caps and the
reversed-order rule for membership of the GPU list; every refusal and its message on the OnDevice stub; the implicit-function formula
of the coupling field against central differences; the names in header, binding and library."""
import os

import numpy as np
import pytest

import _krylov_ref as KR
import _krylov_system_adjoint_ref as SA
import _krylov_system_point_ref as PR
import _krylov_system_ref as SR
import _stencil_ref as R
from _device_helpers import OnDevice
from test_krylov_host import _operator, _raises
from test_krylov_system_host import _operator_of

torch = pytest.importorskip("torch")

PAIRS = [(1, 1), (2, 3), (3, 4), (4, 7)]
_planes = {}


def _oracle_planes(name):
    """The dense planes of a system's cloud from the oracle's coefficients, once."""
    if name not in _planes:
        _planes[name] = SR.oracle_planes(PR.system(name))
    return _planes[name]


@pytest.mark.parametrize("m,nop", PAIRS)
def test_the_stated_orders_against_exact_arithmetic_and_the_dense_matrix(m, nop):
    n = 70
    st = SR.planes_structure(n, 9, nop, seed=7)
    rows = SR.rows_of_structure(st)
    lens = np.array([len(r) for r in rows])
    tlens = np.array([len(r) for r in R.transpose_rows(rows, n)])
    assert any(len({c for c, _ in r}) < len(r) for r in rows) and any(any(c == i for c, _ in r) for i, r in enumerate(rows))
    A = SR.dense_planes(rows, n, nop)
    rng = np.random.default_rng([11, m, nop])
    cpt = rng.standard_normal((m, m, nop, n))
    x = rng.standard_normal((n, m)) * 10.0 ** rng.integers(-2, 3, (n, m))
    for diag in (0.75, rng.standard_normal((m, m)), rng.standard_normal((m, m, n))):
        M = PR.dense_matrix(A, cpt, diag)
        for transposed, chain in ((False, PR.forward_chain(lens, m, nop)), (True, PR.transposed_chain(tlens, m, nop))):
            y = (PR.transposed_product_statement if transposed else PR.product_statement)(rows, cpt, diag, x)
            exact, mag = PR.exact_product(rows, cpt, diag, x, transposed=transposed)
            bound = R.gamma(chain + 2)[:, None] * mag
            assert np.all(np.abs(y - exact) <= bound), (m, nop, transposed)
            dense = ((M.T if transposed else M) @ x.reshape(-1)).reshape(n, m)
            assert np.all(np.abs(dense - exact) <= 4 * R.gamma(m * nop * (tlens if transposed else lens) + m + 2)[:, None] * mag + 1e-300)
        d = PR.jacobi_statement(rows, cpt, diag)
        assert np.all(np.abs(d - np.diag(M)) <= 8 * SR.EPS * (np.abs(SR.diag_blocks(diag, m, n)[range(m), range(m)].T.reshape(-1))
                                                                + np.abs(M).sum(axis=1)))
        assert np.array_equal(KR.jacobi(M.T), KR.jacobi(M))              # the scalar diagonal of M^T is the forward one
    # a table that is constant over the points: the dense matrix and the Jacobi diagonal of the constant-table statements, exactly
    cp = rng.standard_normal((m, m, nop))
    const = PR.constant_table(cp, n)
    assert np.array_equal(PR.dense_matrix(A, const, 0.75), SR.dense_matrix(A, cp, 0.75))
    assert np.array_equal(PR.jacobi_statement(rows, const, 0.75), SR.jacobi_statement(rows, cp, 0.75))
    # the mix is the gradient kernel's u: one chain of m roundings per (o, b)
    z = PR.mix_statement(cpt, x)
    assert z.shape == (n, nop, m)
    assert np.all(np.abs(z - np.einsum("aboi,ia->iob", cpt, x)) <= 2 * R.gamma(m + 1) * np.einsum("aboi,ia->iob", np.abs(cpt), np.abs(x)))


@pytest.mark.parametrize("name", [s for s in PR.SYSTEMS if s.startswith("elasticity")])
def test_a_constant_table_is_the_constant_matrix_exactly(name):
    sy = SR.system(name)
    A = _oracle_planes(name)
    const = PR.constant_table(sy["coupling"], sy["n"])
    assert np.array_equal(PR.elasticity_table(sy["dim"], np.full(sy["n"], SR.MU), np.full(sy["n"], SR.LAMBDA)), const)
    assert np.abs(PR.dense_matrix(A, const, sy["diag"]) - SR.dense_matrix(A, sy["coupling"], sy["diag"])).max() == 0.0


def test_the_systems_are_what_they_say():
    for name in PR.SYSTEMS:
        sy = PR.system(name)
        cpt, n, m, nop = sy["coupling"], sy["n"], sy["m"], sy["nop"]
        assert cpt.shape == (m, m, nop, n) and cpt.flags["C_CONTIGUOUS"]
        f = PR.field(sy["S"])[0]
        if name.startswith("elasticity"):
            mu, lam = 1.0 + 0.5 * f, 1.0 - 0.5 * f
            assert 0.5 <= mu.min() and mu.max() <= 1.5 and np.ptp(mu) > 0.5
            assert np.abs(cpt[0, 0, 0] + (lam + 2.0 * mu)).max() <= 16 * SR.EPS and np.array_equal(cpt[0, 1, 1], -(lam + mu))
            assert np.all(cpt[range(m), range(m), nop - 1] == 1.0)
        else:
            h = n ** -0.5
            k = cpt[0, 0, 0] / (-0.25 * h * h)
            assert (m, nop) == (1, 3) and 0.5 <= k.min() and k.max() <= 1.5 and np.allclose(k, 1.0 + 0.5 * f)
            # k_x and k_y are the derivatives of k: central differences of the field
            e = 1e-6
            for o, step in ((1, [e, 0.0]), (2, [0.0, e])):
                fd = (PR.field(sy["S"] + step)[0] - PR.field(sy["S"] - step)[0]) / (2 * e) * 0.5
                assert np.allclose(cpt[0, 0, o] / (-0.25 * h * h), fd, atol=1e-7)


_dense = {}


def _matrix(name, transposed):
    if name not in _dense:
        sy = PR.system(name)
        _dense[name] = (sy, PR.dense_matrix(_oracle_planes(name), sy["coupling"], sy["diag"]))
    sy, M = _dense[name]
    if transposed:
        return sy, np.ascontiguousarray(M.T), SA.adjoint_rhs(sy["n"], sy["m"]).reshape(-1)
    return sy, M, sy["b"].reshape(-1)


@pytest.fixture(scope="module")
def solved():
    out = {}
    for name, pc, tr in PR.CASES:
        sy, M, b = _matrix(name, tr)
        out[name, pc, tr] = SR.solve_ref(M, b, pc)
        out[name, pc, tr, "reversed"] = SR.solve_ref(M, b, pc, reverse=True)
    return out


@pytest.mark.parametrize("name,pc,transposed", PR.CASES)
def test_reference_converges_within_the_cap_of_the_gpu_tests(solved, name, pc, transposed):
    sy, M, b = _matrix(name, transposed)
    x, its, status, hist = solved[name, pc, transposed]
    cap = (PR.TRANSPOSED_CAPS if transposed else PR.CAPS)[name][pc]
    print("%s %s%s: %d iterations, maxiter %d" % (name, pc, " transposed" if transposed else "", its, cap))
    assert status == KR.CONVERGED
    assert hist[-1] <= KR.RTOL * np.linalg.norm(b)
    assert np.linalg.norm(b - M @ x) <= 2 * KR.RTOL * np.linalg.norm(b)
    assert 0 < its <= cap, "set the cap of (%r, %r, %r) to %d" % (name, pc, transposed, 2 * its)
    assert cap <= 3 * its


@pytest.mark.parametrize("name,pc,transposed", PR.CASES)
def test_reversed_summation_order_moves_the_count_by_less_than_a_quarter(solved, name, pc, transposed):
    its, status = solved[name, pc, transposed][1:3]
    its_r, status_r = solved[name, pc, transposed, "reversed"][1:3]
    ratio = max(its, its_r) / min(its, its_r)
    print("%s %s%s: %d iterations, reversed %d (%.3fx)" % (name, pc, " transposed" if transposed else "", its, its_r, ratio))
    assert status == status_r == KR.CONVERGED
    case = (name, pc, transposed)
    assert (ratio < 1.25) == (case not in PR.HOST_ONLY), "move %r %s HOST_ONLY" % (case, "into" if ratio >= 1.25 else "out of")
    assert set(PR.GPU_CASES) == set(PR.CASES) - set(PR.HOST_ONLY)


@pytest.mark.parametrize("m,nop", PAIRS)
def test_matrix_of_a_host_built_structure_is_the_dense_statement(m, nop):
    import wlsqm.hip as h
    from wlsqm import _binding
    if not os.path.exists(_binding.LIB_PATH):
        return                                                           # the constructor asks the library for the workspace's size
    n = 130
    st = SR.planes_structure(n, 9, nop, seed=13)
    rows = SR.rows_of_structure(st)
    A = SR.dense_planes(rows, n, nop)
    rng = np.random.default_rng([17, m, nop])
    cpt = rng.standard_normal((m, m, nop, n))
    if m > 1:
        cpt[0, 1] = 0.0                                                  # a block without a stencil
    absA = np.stack([R.dense([[(c, np.abs(v)) for c, v in r] for r in rows], n, o) for o in range(nop)])
    scale = np.einsum("aboi,oij->iajb", np.abs(cpt), absA).reshape(m * n, m * n)
    for diag in (0.0, rng.standard_normal((m, m)), rng.standard_normal((m, m, n))):
        held = OnDevice(torch.from_numpy(diag)) if np.ndim(diag) == 3 else diag
        solver = h.StencilSystemSolver(_operator_of(st), OnDevice(torch.from_numpy(cpt)), diag=held)
        assert solver.per_point and (solver.m, solver.nop, solver.npoints) == (m, nop, n)
        solver.coupling = torch.from_numpy(cpt)                          # matrix() indexes them: the stubs have served the checks
        if np.ndim(diag) == 3:
            solver.diag = torch.from_numpy(diag)
        got = solver.matrix()
        assert got.layout == torch.sparse_csr and tuple(got.shape) == (m * n, m * n)
        want = PR.dense_matrix(A, cpt, diag)
        assert np.all(np.abs(got.to_dense().numpy() - want) <= 4 * nop * np.finfo(np.float64).eps * scale)
        if m > 1:
            dense = got.to_dense().numpy().reshape(n, m, n, m)
            assert np.array_equal(dense[:, 0, :, 1] != 0.0, np.eye(n, dtype=bool) & (np.ndim(diag) > 0))
        assert solver.memory_used() == _binding.lib().wlsqm_hip_krylov_system_workspace_bytes(n, m)
        solver.close()


def test_refusals_and_argument_checks_need_no_device():
    import wlsqm.hip as h
    from wlsqm import _binding
    D = OnDevice
    f64 = torch.float64
    n = 130
    op = _operator(n)                                                    # two value planes
    S = h.StencilSystemSolver
    z = lambda *shape: torch.zeros(shape, dtype=f64)
    cpt = z(2, 2, 2, n)
    # the constructor: a device tensor of four dimensions is a per-point table; of any other rank it is refused as before
    _raises("coupling must be a host array \\(m, m, nop\\); got a device tensor", S, op, D(z(2, 2, 2)))
    _raises("coupling must be a host array \\(m, m, nop\\); got a device tensor", S, op, D(z(2, 2, 2, n, 1)))
    shape = ("a per-point coupling must be a contiguous float64 device tensor of shape \\(m, m, nop, npoints\\) with 1 <= m <= 4, nop = 2, "
             "the operator's value planes, and npoints = 130; got shape ")
    _raises(shape + "\\(2, 2, 2, 131\\)", S, op, D(z(2, 2, 2, n + 1)))
    _raises(shape + "\\(2, 2, 3, 130\\)", S, op, D(z(2, 2, 3, n)))
    _raises(shape + "\\(2, 3, 2, 130\\)", S, op, D(z(2, 3, 2, n)))
    _raises(shape + "\\(5, 5, 2, 130\\)", S, op, D(z(5, 5, 2, n)))
    _raises(shape + "\\(0, 0, 2, 130\\)", S, op, D(z(0, 0, 2, n)))
    _raises(shape + "\\(2, 2, 2, 130\\) with strides \\(4, 2, 1, 8\\)", S, op, D(z(n, 2, 2, 2).permute(1, 2, 3, 0)))
    _raises("expected 'float64'.*argument coupling", S, op, D(torch.zeros((2, 2, 2, n))))
    for bad in (h.BlockJacobi(16), h.ApproximateInverse(), "ilu"):
        _raises("preconditioner must be 'jacobi' or None", S, op, D(cpt), preconditioner=bad)
    _raises("diag must be a contiguous float64 device tensor of shape \\(2, 2, 130\\); got shape \\(2, 2, 131\\)", S, op, D(cpt),
            diag=D(z(2, 2, n + 1)))
    with pytest.raises(TypeError):
        S(op, D(cpt), method="bicgstab2")
    with pytest.raises(TypeError):
        S(op, D(cpt), nfields=2)
    if not os.path.exists(_binding.LIB_PATH):
        return
    diag = torch.ones((2, 2, n), dtype=f64)
    solver = S(op, D(cpt), diag=D(diag), preconditioner=None)
    assert solver.per_point and (solver.m, solver.nop, solver.npoints) == (2, 2, n) and solver.refresh() is solver
    assert solver._cp is None and solver._mixed is None
    host = S(op, np.ones((2, 2, 2)), preconditioner=None)
    assert not host.per_point

    # set_coupling: the same kind, the same shape
    kind = "set_coupling cannot change the kind of table: the solver was made with "
    _raises(kind + "a per-point device tensor \\(m, m, nop, npoints\\)", solver.set_coupling, np.ones((2, 2, 2)))
    _raises(kind + "a per-point device tensor", solver.set_coupling, D(z(2, 2, 2)))
    _raises(kind + "a host table \\(m, m, nop\\)", host.set_coupling, D(cpt))
    _raises("coupling must be a host array \\(m, m, nop\\); got a device tensor", host.set_coupling, D(z(2, 2, 2)))
    _raises(shape + "\\(2, 2, 2, 129\\)", solver.set_coupling, D(z(2, 2, 2, n - 1)))
    _raises("the new coupling must keep the solver's shape \\(2, 2, 2, 130\\); got shape \\(3, 3, 2, 130\\)", solver.set_coupling,
            D(z(3, 3, 2, n)))
    other = D(z(2, 2, 2, n))
    assert solver.set_coupling(other) is solver and solver.coupling is other

    # the tensor joins the overlap checks
    b, x, lam = z(n, 2), z(n, 2), z(n, 2)
    both = z(2 * n + 1, 2)
    inside = D(other.view(-1)[:2 * n].view(n, 2))
    for call in (solver.solve, lambda b_, x_, **kw: solver.enqueue(b_, x_, 5, **kw)):
        _raises("x overlaps coupling", call, D(b), inside)
        _raises("b overlaps coupling", call, inside, D(x))
        _raises("b overlaps x", call, D(both[:n]), D(both[n - 1:2 * n - 1]), transpose=True)
        _raises("x overlaps diag", call, D(b), D(diag.view(-1)[:2 * n].view(n, 2)))
        _raises("rtol and atol must be finite and >= 0", call, D(b), D(x), rtol=-1.0)
    _raises("out overlaps coupling", solver.product, D(b), out=inside)
    _raises("x must be 16-byte aligned for m = 2", solver.solve, D(b), D(both.view(-1)[1:1 + 2 * n].view(n, 2)))
    G = solver.gradients
    _raises("lam overlaps coupling", G, inside, D(x), diag=True)
    _raises("grad_diag overlaps coupling", G, D(lam), D(x), diag=D(other.view(-1)[:4 * n].view(2, 2, n)))
    total = op._m["total"]
    room = z(2 * total + 8 * n)
    solver.set_coupling(D(room[2 * total - 8:2 * total - 8 + 8 * n].view(2, 2, 2, n)))
    _raises("values overlaps coupling", G, D(lam), D(x), values=D(room[:2 * total].view(2, total)))
    solver.set_coupling(other)
    _raises("lam overlaps coupling", solver.coupling_gradient, inside, D(x))
    assert op._t is None and solver._mixed is None                       # nothing is built for a refused call

    # differentiable_stencil_system_solve
    F = h.differentiable_stencil_system_solve
    _raises("coupling must be a float64 torch tensor \\(m, m, nop\\), on the host or on the device", F, solver, D(b), coupling=np.ones((2, 2, 2, n)))
    _raises("argument coupling must be a device", F, solver, D(b), coupling=z(2, 2, 2, n))
    _raises("wrong number of dimensions.*argument coupling", F, solver, D(b), coupling=D(z(2, 2, 2)))
    _raises(shape + "\\(2, 2, 2, 131\\)", F, solver, D(b), coupling=D(z(2, 2, 2, n + 1)))
    _raises("expected 'float64'.*argument coupling", F, solver, D(b), coupling=D(torch.zeros((2, 2, 2, n))))
    _raises("coupling must be a float64 torch tensor of shape \\(2, 2, 2\\)", F, host, D(b), coupling=z(2, 2, 2, n))
    _raises("argument b must be a device", F, solver, b)
    solver.close()
    solver.close()
    assert solver.coupling is None
    for call in (lambda: solver.solve(D(b), D(x)), lambda: solver.set_coupling(other), solver.memory_used, solver.prepare_transpose,
                 solver.matrix, lambda: solver.coupling_gradient(D(lam), D(x)), lambda: F(solver, D(b))):
        _raises("the stencil system solver has been closed", call)
    host.close()


def test_sharded_has_no_coupled_fields():
    """wlsqm.sharded carries no StencilSystemSolver: a per-point coupling does not change that."""
    import wlsqm.sharded as sh
    assert not any("System" in name for name in dir(sh))


def test_the_coupling_field_formula_against_central_differences():
    """dL/dc[a, b, o, i] = -lam[i, a] (A_o x[:, b])_i along a random unit direction, by dense solves on a random system."""
    sy = SR.system("random-m3")
    n, m, nop = sy["n"], sy["m"], sy["nop"]
    A = SR.oracle_planes(sy)
    rng = np.random.default_rng([83, n, m])
    cpt = PR.constant_table(sy["coupling"], n) * (1.0 + 0.3 * rng.standard_normal((m, m, nop, n)))
    w = SA.adjoint_rhs(n, m)
    G = PR.implicit_gradients(A, cpt, sy["diag"], sy["b"], w)
    u = rng.standard_normal(cpt.shape)
    u /= np.linalg.norm(u)
    loss = lambda t: SA.refined_loss(w.reshape(-1), PR.dense_matrix(A, cpt + t * u, sy["diag"]), sy["b"].reshape(-1))
    formula = float((G["coupling"] * u).sum())
    rel = [abs(SA.central(loss, h) - formula) / abs(formula) for h in (1e-5, 1e-6)]
    print("coupling field: formula %.12e, relative distance %.2e (h = 1e-5), %.2e (h = 1e-6)" % (formula, rel[0], rel[1]))
    assert min(rel) <= SA.FD_BAR
    # its sum over the points is the constant table's gradient
    const = SA.implicit_gradients(A, sy["coupling"], sy["diag"], sy["b"], w)
    field = PR.implicit_gradients(A, PR.constant_table(sy["coupling"], n), sy["diag"], sy["b"], w)
    assert np.allclose(field["coupling"].sum(axis=-1), const["coupling"], rtol=1e-12, atol=1e-12 * np.abs(const["coupling"]).max())


def test_header_binding_and_library_name_the_entry_points():
    import subprocess
    from wlsqm import _binding
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "wlsqm_hip.h")).read()
    binding = open(os.path.join(root, "python-wlsqm_amd", "wlsqm", "_binding.py")).read()
    source = open(os.path.join(root, "python-wlsqm_amd", "csrc", "krylov.hip")).read()
    names = ["wlsqm_hip_krylov_system_point_%s_device" % s for s in ("start", "bicgstab", "product", "grads")]
    for name in names:
        assert " %s(" % name in header
    assert '"wlsqm_hip_krylov_system_point_%s_device"' in binding
    for kernel in ("krylov-system-spmv-point", "krylov-system-diag-point", "krylov-system-mix", "krylov-system-spmv-mixed"):
        assert '"%s"' % kernel in header
    for kernel in ("krylov-system-spmv-point", "krylov-system-diag-point", "krylov-system-spmv-mixed"):
        assert '"%s"' % kernel in source
    # the existing entry points keep their signatures: the declarations of sections 24 and 25 stand word for word
    assert ("int wlsqm_hip_krylov_system_product_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width, "
            "const int64_t* soff,\n") in header
    if os.path.exists(_binding.LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", _binding.LIB_PATH], capture_output=True, text=True).stdout
        for name in names:
            assert " T %s" % name in syms
        L = _binding.lib()
        assert len(L.wlsqm_hip_krylov_system_point_start_device.argtypes) == len(L.wlsqm_hip_krylov_system_start_device.argtypes) + 2
        assert len(L.wlsqm_hip_krylov_system_point_product_device.argtypes) == len(L.wlsqm_hip_krylov_system_product_device.argtypes) + 2
        assert L.wlsqm_hip_krylov_system_point_grads_device.argtypes == L.wlsqm_hip_krylov_system_grads_device.argtypes
        # the C side checks again and answers a status: no device is touched by a refused call
        ws = torch.zeros(4096, dtype=torch.float64)
        i32, i64 = torch.zeros(64, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)
        p = lambda t: t.data_ptr()
        base = [64, 1, p(i32), p(i32), p(i64), p(i32), p(ws), 0]
        tail = [p(ws), p(ws), p(ws), p(ws), 0, None]
        fn = L.wlsqm_hip_krylov_system_point_product_device
        assert fn(*base, 2, 5, p(ws), None, p(ws), 0, None, *tail) != 0 and b"m must be 1 .. 4" in L.wlsqm_hip_last_error()
        assert fn(*base, 9, 2, p(ws), None, p(ws), 0, None, *tail) != 0 and b"nop must be 1 .. 8" in L.wlsqm_hip_last_error()
        assert fn(*base, 2, 2, None, None, p(ws), 0, None, *tail) != 0 and b"null array" in L.wlsqm_hip_last_error()
        assert fn(*base, 2, 2, p(ws), None, p(ws), 1, None, *tail) != 0 and b"null array" in L.wlsqm_hip_last_error()
        assert fn(*base, 2, 2, p(ws) + 4, None, p(ws), 0, None, *tail) != 0 and b"8-byte aligned" in L.wlsqm_hip_last_error()
        assert fn(*base, 2, 2, p(ws), None, p(ws), 1, p(ws) + 8, *tail) != 0 and b"16-byte aligned" in L.wlsqm_hip_last_error()
        assert fn(*base[:1], 0, *base[2:], 2, 2, p(ws), None, p(ws), 0, None, *tail) != 0 and b"npoints must be" in L.wlsqm_hip_last_error()
