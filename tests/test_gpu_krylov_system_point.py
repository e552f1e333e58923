"""GPU tests of coupled solves with a per-point coupling (wlsqm.hip.StencilSystemSolver with a device tensor (m, m, nop, npoints),
csrc/krylov.hip's krylov_system_spmv_point / diag_point / mix / spmv_mixed kernels and the per-point form of krylov_system_grads,
DESIGN.md section 26).

  1. the forward and the transposed product against the exact value of the dense statement: an unknown within gamma_{T + 2} of the
     sum of the magnitudes of its terms, T the longest chain of roundings a term passes through in the stated order
     (tests/_krylov_system_point_ref.forward_chain: len + m nop + 1; transposed_chain: m + nop len + 1); both dot products within
     section 24's bound; up to 65 points bit for bit the stated order, the mixed plane z included;
  2. a table that is constant over the points against the constant-table solver on the same operator, within the sum of the two
     bounds; that solver's bits, workspace and kernel families unchanged with a per-point solver at work beside it;
  3. solves of tests/_krylov_system_point_ref.GPU_CASES, forward and transposed, by section 17's criteria within the caps;
  4. bit for bit: twice, check_every=1 against one enqueue, eager against a captured op.update + enqueue, a captured enqueue replayed
     after coupling.copy_(new);
  5. statuses, never a fault;
  6. gradients: coupling_gradient per point, its sum over the points, the gradient kernel bit for bit its statement, and
     differentiable_stencil_system_solve to b, diag, coupling, coefficients and S against the dense implicit-function gradients."""
import math
from fractions import Fraction

import numpy as np
import pytest

import _krylov_ref as KR
import _krylov_system_adjoint_ref as SA
import _krylov_system_point_ref as PR
import _krylov_system_ref as SR
import _stencil_ref as R
from _device_helpers import bits, dev as _t, nan as _nan, same_bits as _same_bits, wlsqm  # noqa: F401 (fixture)
from test_gpu_krylov_system import PAIRS, PRODUCT_CASES, _diag, _held_to_the_reference, _operator

pytestmark = pytest.mark.gpu


def _zeros(n, m):
    import torch
    return torch.zeros((n, m), dtype=torch.float64, device="cuda")


# ---- 1. the products and their dots ---------------------------------------------------------------------------------------------------------

def _dots_within_section_24(nrows, m, v, pairs):
    """Both dot products within gamma_{m n + depth} sum |a_i b_i| (tests/test_gpu_krylov_system.py); returns the worst share."""
    nwg = (nrows + 255) // 256
    depth = (m - 1) + 6 + 3 + math.ceil(nwg / 256) + 6 + 3
    worst = 0.0
    for got_dot, other in pairs:
        ex, mg = KR.exact_dot(v, other)
        bnd = float(R.gamma(m * nrows + depth)) * float(mg)
        worst = max(worst, float(abs(Fraction(got_dot) - ex) / Fraction(bnd))) if bnd > 0 else worst
        assert abs(Fraction(got_dot) - ex) <= bnd, (nrows, m, got_dot, float(ex), bnd)
    return worst


@pytest.mark.parametrize("nrows,m,nop,form", PRODUCT_CASES)
def test_products_and_dots_against_exact_arithmetic(wlsqm, nrows, m, nop, form):
    import torch
    import wlsqm.hip as whip
    st = SR.planes_structure(nrows, 9, nop, seed=31)
    rows = SR.rows_of_structure(st)
    trows = R.transpose_rows(rows, nrows)
    lens, tlens = np.array([len(r) for r in rows]), np.array([len(r) for r in trows])
    if nrows >= 130:
        assert lens.min() == 0 and np.all(lens[64:128] == 0)            # empty rows and an empty slice
    assert any(len({c for c, _ in r}) < len(r) for r in rows) and any(any(c == i for c, _ in r) for i, r in enumerate(rows))
    rng = np.random.default_rng([97, nrows, m, nop])
    cpt = rng.standard_normal((m, m, nop, nrows))
    x = rng.standard_normal((nrows, m)) * 10.0 ** rng.integers(-2, 3, (nrows, m))
    w = rng.standard_normal((nrows, m))
    held, d = _diag(form, m, nrows, rng)
    op = _operator(whip, st)
    coupling = _t(cpt)
    solver = whip.StencilSystemSolver(op, coupling, diag=held)
    assert solver.per_point and solver.coupling is coupling
    check = np.arange(nrows) if nrows <= 300 else np.r_[0:40, 32750:32790, nrows - 40:nrows]
    for transposed in (False, True):
        out = _nan(nrows, m)
        got, dot_w, dot_v = solver.product(_t(x), _t(w), out=out, transpose=transposed)
        assert got is out and whip.last_kernel() == ("krylov-system-spmv-mixed" if transposed else "krylov-system-spmv-point")
        v = got.cpu().numpy()
        assert np.isfinite(v).all()
        exact, mag = PR.exact_product(rows, cpt, d, x, check, transposed=transposed, trows=trows)
        chain = PR.transposed_chain(tlens[check], m, nop) if transposed else PR.forward_chain(lens[check], m, nop)
        bound = R.gamma(chain + 2)[:, None] * mag
        err = np.abs(v[check] - exact)
        share = float((err / np.maximum(bound, 1e-300)).max())
        assert np.all(err <= bound), (nrows, m, nop, form, transposed, share)
        if nrows <= 65:
            statement = PR.transposed_product_statement if transposed else PR.product_statement
            assert _same_bits(v, statement(rows, cpt, d, x))
            if transposed:
                assert tuple(solver._mixed.shape) == (nrows, nop, m) and _same_bits(solver._mixed.cpu().numpy(), PR.mix_statement(cpt, x))
        worst_dot = _dots_within_section_24(nrows, m, v, ((dot_w, w), (dot_v, v)))
        print("n %d m %d nop %d %s%s: v at %.3f of its bound, the dots at %.3g of theirs"
              % (nrows, m, nop, form, " transposed" if transposed else "", share, worst_dot))
        again, dw2, dv2 = solver.product(_t(x), _t(w), transpose=transposed)
        assert torch.equal(bits(again), bits(got)) and (dw2, dv2) == (dot_w, dot_v)
    assert solver.memory_used() == 8 * (solver._ws.numel() + m * nop * nrows)  # the mixed plane is counted once it exists
    solver.close(); op.close()


# ---- 2. a table that is constant over the points ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,nop", PAIRS)
def test_a_constant_table_against_the_constant_solver(wlsqm, m, nop):
    import torch
    import wlsqm.hip as whip
    from wlsqm import _binding
    n = 300
    st = SR.planes_structure(n, 9, nop, seed=43)
    rows = SR.rows_of_structure(st)
    trows = R.transpose_rows(rows, n)
    lens, tlens = np.array([len(r) for r in rows]), np.array([len(r) for r in trows])
    rng = np.random.default_rng([101, m, nop])
    cp = rng.standard_normal((m, m, nop))
    dom = 1.0 + 1.5 * np.abs(SR.dense_matrix(SR.dense_planes(rows, n, nop), cp, 0.0)).sum(axis=1).reshape(n, m)
    d = np.zeros((m, m, n))
    d[range(m), range(m)] = dom.T                                        # diagonally dominant: the solves below converge
    x, b = rng.standard_normal((n, m)), rng.standard_normal((n, m))
    op = _operator(whip, st)
    const = whip.StencilSystemSolver(op, cp, diag=_t(d))

    def constant_run():
        xs = _zeros(n, m)
        info = const.solve(_t(b), xs, maxiter=200)
        after_solve = whip.last_kernel()
        prod = const.product(_t(x))
        after_product = whip.last_kernel()
        lam = _zeros(n, m)
        info_t = const.solve(_t(b), lam, maxiter=200, transpose=True)
        return info, xs, after_solve, after_product, prod[0], prod[1:], info_t, lam, const.memory_used()

    ref = constant_run()
    assert ref[0].status == ref[6].status == 0 and ref[2:4] == ("krylov-update", "krylov-system-spmv")
    assert ref[8] == _binding.lib().wlsqm_hip_krylov_system_workspace_bytes(n, m)
    point = whip.StencilSystemSolver(op, _t(PR.constant_table(cp, n)), diag=_t(d))
    exact, mag = SR.exact_product(rows, cp, d, x)
    for transposed in (False, True):
        got = point.product(_t(x), transpose=transposed)[0].cpu().numpy()
        want = const.product(_t(x), transpose=transposed)[0].cpu().numpy()
        if transposed:
            exact, mag = PR.exact_product(rows, PR.constant_table(cp, n), d, x, transposed=True)
            ln, chain = tlens, PR.transposed_chain(tlens, m, nop)
        else:
            ln, chain = lens, PR.forward_chain(lens, m, nop)
        both = (R.gamma(chain + 2) + R.gamma(m * nop * ln + m + 2))[:, None] * mag
        assert np.all(np.abs(got - want) <= both), (m, nop, transposed)
        assert np.all(np.abs(got - exact) <= R.gamma(chain + 2)[:, None] * mag)
    xp = _zeros(n, m)
    info_p = point.solve(_t(b), xp, maxiter=200)
    assert info_p.status == 0 and whip.last_kernel() == "krylov-update"
    point.enqueue(_t(b), _zeros(n, m), 3, transpose=True)               # stopped short, then the constant solver runs whole solves
    beside = constant_run()
    point.product(_t(x))
    after = constant_run()
    for got in (beside, after):
        assert got[0] == ref[0] and torch.equal(bits(got[1]), bits(ref[1])) and got[2:4] == ref[2:4]
        assert torch.equal(bits(got[4]), bits(ref[4])) and got[5] == ref[5] and got[6] == ref[6]
        assert torch.equal(bits(got[7]), bits(ref[7])) and got[8] == ref[8]
    Mflat = const.matrix().to_dense().cpu().numpy()
    assert np.abs(point.matrix().to_dense().cpu().numpy() - Mflat).max() <= 4 * nop * np.finfo(np.float64).eps * np.abs(Mflat).max()
    assert np.linalg.norm(b.reshape(-1) - Mflat @ xp.cpu().numpy().reshape(-1)) <= 2 * KR.RTOL * np.linalg.norm(b)
    const.close(); point.close(); op.close()


# ---- 3. solves ------------------------------------------------------------------------------------------------------------------------------

_made = {}


def _system(name):
    """The per-point system `name` on the device and what the tests share about it, computed once and left unchanged."""
    if name not in _made:
        import wlsqm.hip as whip
        sy = PR.system(name)
        op = whip.StencilOperator(sy["dim"], sy["order"], _t(sy["S"]), _t(sy["hoods"]), _t(sy["nk"]), _t(sy["knowns"]), _t(sy["wm"]),
                                  _t(sy["rows"]))
        A = np.stack([op.to_sparse_csr(o).to_dense().cpu().numpy() for o in range(sy["nop"])])
        M = PR.dense_matrix(A, sy["coupling"], sy["diag"])
        _made[name] = dict(sy=sy, op=op, A=A, M=M, coupling=_t(sy["coupling"]), kappa=np.linalg.cond(M), sides={}, solvers={})
    return _made[name]


def _side(m, transposed):
    """The dict that test_gpu_krylov_system._held_to_the_reference takes, for M or for M^T."""
    if transposed not in m["sides"]:
        sy = m["sy"]
        M = np.ascontiguousarray(m["M"].T) if transposed else m["M"]
        b = SA.adjoint_rhs(sy["n"], sy["m"]) if transposed else sy["b"]
        bf = b.reshape(-1)
        m["sides"][transposed] = dict(M=M, b=_t(b), bflat=bf, xstar=np.linalg.solve(M, bf), stop=KR.RTOL * np.linalg.norm(bf), kappa=m["kappa"])
    return m["sides"][transposed]


def _solver(m, pc):
    import wlsqm.hip as whip
    if pc not in m["solvers"]:
        m["solvers"][pc] = whip.StencilSystemSolver(m["op"], m["coupling"], diag=m["sy"]["diag"], preconditioner=pc)
    return m["solvers"][pc]


@pytest.mark.parametrize("name,pc,transposed", PR.GPU_CASES)
def test_solve(wlsqm, name, pc, transposed):
    import wlsqm.hip as whip
    m = _system(name)
    side, solver = _side(m, transposed), _solver(m, pc)
    cap = (PR.TRANSPOSED_CAPS if transposed else PR.CAPS)[name][pc]
    info = solver.solve(side["b"], rtol=KR.RTOL, maxiter=cap, transpose=transposed)
    x = solver.x
    assert tuple(x.shape) == (m["sy"]["n"], m["sy"]["m"]) and whip.last_kernel() == "krylov-update"
    _held_to_the_reference(side, x.cpu().numpy().reshape(-1), info, None, pc, cap, "%s %s%s" % (name, pc, " transposed" if transposed else ""))


def test_solve_from_a_guess_with_a_diag_tensor(wlsqm):
    """A non-zero x0 and a per-point diag tensor (ones: the matrix of diag = 1.0, so the reference count behind the cap stands; a
    random start of unit size is no further from the solution than zero is by more than the cap's factor of two)."""
    import wlsqm.hip as whip
    name = "diffusion-2D-n130"
    m = _system(name)
    sy, side = m["sy"], _side(m, False)
    n, mm = sy["n"], sy["m"]
    solver = whip.StencilSystemSolver(m["op"], m["coupling"], diag=_t(np.ones((mm, mm, n))))
    x0 = np.random.default_rng([67, n]).standard_normal((n, mm))
    x = _t(x0)
    cap = PR.CAPS[name]["jacobi"]
    info = solver.solve(side["b"], x, rtol=KR.RTOL, maxiter=cap, check_every=3)
    assert solver.x is x
    _held_to_the_reference(side, x.cpu().numpy().reshape(-1), info, x0.reshape(-1), "jacobi", cap, name + " from a guess")
    solver.close()


# ---- 4. bit for bit -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("transposed", (False, True))
def test_same_bits_twice_and_behind_the_stop(wlsqm, transposed):
    import torch
    name = "elasticity-2D-n130"
    m = _system(name)
    sy, solver, b = m["sy"], _solver(m, "jacobi"), _side(m, transposed)["b"]
    cap = (PR.TRANSPOSED_CAPS if transposed else PR.CAPS)[name]["jacobi"]
    solver.prepare_transpose()
    runs = []
    for check_every in (8, 8, 1):
        x = _zeros(sy["n"], sy["m"])
        runs.append((solver.solve(b, x, maxiter=cap, check_every=check_every, transpose=transposed), x))
    assert runs[0][0] == runs[1][0] == runs[2][0] and runs[0][0].status == 0
    assert torch.equal(bits(runs[0][1]), bits(runs[1][1])) and torch.equal(bits(runs[0][1]), bits(runs[2][1]))
    k = runs[2][0].iterations
    x = _zeros(sy["n"], sy["m"])
    before = torch.cuda.memory_allocated()
    solver.enqueue(b, x, k + 5, transpose=transposed)                    # the five behind the stop leave x and the scalars alone
    assert torch.cuda.memory_allocated() == before
    assert solver.info() == runs[2][0] and torch.equal(bits(x), bits(runs[2][1]))
    x = _zeros(sy["n"], sy["m"])
    solver.enqueue(b, x, k - 1, transpose=transposed)                    # one too few: the early exit is not what made them agree
    assert solver.info().status == KR.MAXITER and solver.info().iterations == k - 1
    assert not torch.equal(bits(x), bits(runs[2][1]))


def test_capture_behind_update_and_a_changed_coupling(wlsqm):
    import torch
    import wlsqm.hip as whip
    name = "diffusion-2D-n130"
    sy = PR.system(name)
    n, m = sy["n"], sy["m"]
    rng = np.random.default_rng(41)
    SA_, SB = sy["S"], sy["S"] + 0.05 * n ** -0.5 * rng.standard_normal(sy["S"].shape)
    CA, CB = sy["coupling"], sy["coupling"] * (1.0 + 0.2 * rng.random(sy["coupling"].shape))
    S, coupling = _t(SA_), _t(CA)
    op = whip.StencilOperator(2, 2, S, _t(sy["hoods"]), _t(sy["nk"]), _t(sy["knowns"]), _t(sy["wm"]), _t(sy["rows"]))
    solver = whip.StencilSystemSolver(op, coupling, diag=sy["diag"])
    b, x0 = _t(sy["b"]), _t(rng.standard_normal((n, m)))
    x = _nan(n, m)
    iters = 2 * PR.CAPS[name]["jacobi"]                                  # a count to enqueue, not a bound

    def step(transpose=False):
        x.copy_(x0)
        op.update(S, check=False)
        solver.enqueue(b, x, iters, transpose=transpose)

    def eager(s, c, transpose=False):
        S.copy_(_t(s)); coupling.copy_(_t(c))
        step(transpose)
        return x.clone(), solver.info()

    at_aa, info_aa = eager(SA_, CA)
    at_ba, info_ba = eager(SB, CA)
    at_ab, info_ab = eager(SA_, CB)
    assert info_aa.status == info_ba.status == info_ab.status == 0
    assert not torch.equal(bits(at_aa), bits(at_ba)) and not torch.equal(bits(at_aa), bits(at_ab))
    S.copy_(_t(SA_)); coupling.copy_(_t(CA))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        step()
    torch.cuda.synchronize()
    for s, c, want, info in ((SA_, CA, at_aa, info_aa), (SB, CA, at_ba, info_ba), (SA_, CB, at_ab, info_ab)):
        S.copy_(_t(s)); coupling.copy_(_t(c))                            # the captured graph reads the changed tensors
        x.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(x), bits(want)) and solver.info() == info
    # the transposed enqueue: refused inside a capture until the mixed plane exists, then captured and replayed after coupling.copy_
    assert solver._mixed is None
    refused = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="the stream is capturing: call prepare_transpose before the capture"):
        with torch.cuda.graph(refused, stream=torch.cuda.Stream()):
            solver.enqueue(b, x, iters, transpose=True)
    torch.cuda.synchronize()
    assert solver.prepare_transpose() is True and solver.prepare_transpose() is False and solver._mixed is not None
    t_a, tinfo_a = eager(SA_, CA, True)
    t_b, tinfo_b = eager(SA_, CB, True)
    assert tinfo_a.status == tinfo_b.status == 0 and not torch.equal(bits(t_a), bits(t_b)) and not torch.equal(bits(t_a), bits(at_aa))
    coupling.copy_(_t(CA))
    tgraph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(tgraph, stream=torch.cuda.Stream()):
        step(True)
    torch.cuda.synchronize()
    coupling.copy_(_t(CB))
    x.fill_(float("nan"))
    tgraph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(x), bits(t_b)) and solver.info() == tinfo_b
    # set_coupling: another tensor, the next eager solve reads it
    other = _t(CB)
    assert solver.set_coupling(other) is solver and solver.coupling is other
    x.copy_(x0)
    assert solver.solve(b, x, maxiter=iters) == info_ab and torch.equal(bits(x), bits(at_ab))
    solver.close(); op.close()


# ---- 5. statuses, not faults ----------------------------------------------------------------------------------------------------------------

def test_statuses(wlsqm):
    import torch
    import wlsqm.hip as whip
    sy = SR.system("random-m3")
    n, mm, nop = sy["n"], sy["m"], sy["nop"]
    cpt = PR.constant_table(sy["coupling"], n) * (1.0 + 0.1 * np.random.default_rng(103).random((mm, mm, nop, n)))
    # the diagonal of `diag` dominates the constant table's rows by 1.5: a table within 1.1 of it keeps the system dominant
    # the point whose coefficients go bad has stored entries: M^T applies a point's coefficients to the entries of its own row, so those
    # of an empty row are never read there (M reads them: NaN * 0)
    bad = next(i for i, r in enumerate(SR.rows_of_structure(sy["st"])) if len(r) > 1)
    op = _operator(whip, sy["st"])
    b = _t(sy["b"])
    x0 = np.random.default_rng(71).standard_normal((n, mm))
    for pc in ("jacobi", None):
        coupling = _t(cpt)
        solver = whip.StencilSystemSolver(op, coupling, diag=_t(sy["diag"]), preconditioner=pc)
        for transposed in (False, True):
            x = _zeros(n, mm)
            info = solver.solve(_zeros(n, mm), x, transpose=transposed)  # b = 0 from x = 0: converged before the first iteration
            assert (info.status, info.iterations, info.residual) == (0, 0, 0.0) and torch.all(x == 0.0)
            x = _t(x0)
            info = solver.solve(b, x, maxiter=0, transpose=transposed)
            assert (info.status, info.iterations) == (KR.MAXITER, 0) and _same_bits(x.cpu().numpy(), x0)
            bn = b.clone()
            bn[3, 1] = float("nan")
            x = _t(x0)
            info = solver.solve(bn, x, transpose=transposed)
            assert info.status == KR.NONFINITE and info.iterations == 0 and _same_bits(x.cpu().numpy(), x0)
            x = _zeros(n, mm)
            assert solver.solve(b, x, maxiter=400, transpose=transposed).status == 0
            # a NaN in the coupling tensor of one point: the scalar diagonal of that point is unusable (status 4) with Jacobi, the
            # residual is not finite (status 3) without; x as given either way
            coupling[:, :, :, bad] = float("nan")
            x = _t(x0)
            info = solver.solve(b, x, transpose=transposed)
            assert info.status == (KR.DIAGONAL if pc == "jacobi" else KR.NONFINITE) and info.iterations == 0
            assert _same_bits(x.cpu().numpy(), x0)
            coupling.copy_(_t(cpt))
        solver.close()
    # a zero coupled diagonal: unknown (5, 1) has D_11 = 0 and no own entry
    st = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in sy["st"].items()}
    st["nk"][5], st["own_mask"][5] = 0, False
    op0 = _operator(whip, st)
    d = sy["diag"].copy()
    d[1, 1, 5] = 0.0
    zero_diag = whip.StencilSystemSolver(op0, _t(cpt), diag=_t(d))
    for transposed in (False, True):
        x = _t(x0)
        info = zero_diag.solve(b, x, transpose=transposed)
        assert info.status == KR.DIAGONAL and info.iterations == 0 and _same_bits(x.cpu().numpy(), x0)
    zero_diag.close(); op0.close(); op.close()


# ---- 6. gradients -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nrows,m,nop", [(n, m, nop) for n in (65, 300) for m, nop in PAIRS] + [(1, 2, 3), (64, 3, 1), (65537, 3, 7), (65537, 4, 4)])
def test_grads_kernel_bit_for_bit_its_statement(wlsqm, nrows, m, nop):
    import torch
    import wlsqm.hip as whip
    st = SR.planes_structure(nrows, 9, nop, seed=31)
    op = _operator(whip, st)
    sell = {k: op._m[k].cpu().numpy() for k in ("len", "width", "soff", "col")}
    total = op._m["total"]
    rng = np.random.default_rng([107, nrows, m, nop])
    cpt = rng.standard_normal((m, m, nop, nrows))
    lam = rng.standard_normal((nrows, m)) * 10.0 ** rng.integers(-2, 3, (nrows, m))
    x = rng.standard_normal((nrows, m)) * 10.0 ** rng.integers(-2, 3, (nrows, m))
    solver = whip.StencilSystemSolver(op, _t(cpt), diag=0.75)
    lam_t, x_t = _t(lam), _t(x)
    got = solver.gradients(lam_t, x_t, values=True, diag=True)
    assert whip.last_kernel() == "krylov-system-grads"
    assert tuple(got.values.shape) == (nop, total) and tuple(got.diag.shape) == (m, m, nrows)
    values, diag = got.values.cpu().numpy(), got.diag.cpu().numpy()
    row, at_all = SA.entries_of(sell, nrows)
    padding = np.ones(total, bool)
    padding[at_all] = False
    assert not values[:, padding].view(np.uint64).any()                  # +0.0 with its sign in every padding position
    check = None if nrows <= 300 else np.unique(np.r_[0:64, rng.integers(64, nrows - 1, 40), 64 * ((nrows - 1) // 64):nrows])
    at, want_values, want_diag = PR.grads_statement(sell, nrows, cpt, lam, x, check)
    assert len(at) > 0 or nrows == 1
    assert _same_bits(values[:, at], want_values)
    assert _same_bits(diag if check is None else diag[:, :, check], want_diag)
    if check is not None:        # everywhere else the dense formula: the chains' 2 m roundings, and numpy's m^2 products and their sum
        c = sell["col"][at_all]
        U = np.einsum("aboj,ja->jbo", cpt, lam)
        dense = -np.einsum("jbo,jb->oj", U[row], x[c])
        mag = np.einsum("aboj,ja,jb->oj", np.abs(cpt)[..., row], np.abs(lam[row]), np.abs(x[c]))
        assert np.all(np.abs(values[:, at_all] - dense) <= float(R.gamma(2 * m) + R.gamma(m * m + 2)) * mag)
    alone = (solver.gradients(lam_t, x_t, values=True), solver.gradients(lam_t, x_t, diag=True))
    assert alone[0].diag is None and alone[1].values is None
    assert torch.equal(bits(alone[0].values), bits(got.values)) and torch.equal(bits(alone[1].diag), bits(got.diag))
    solver.close(); op.close()


@pytest.mark.parametrize("m,nop", PAIRS)
def test_coupling_gradient_per_point_and_its_sum(wlsqm, m, nop):
    """(a, b, o, i): -(lam[i, a] * (A_o x[:, b])_i).  The product A_o x is a chain of len fma in some order: within gamma_{len + 1};
    the multiplication by lam adds one rounding.  Its sum over n points against the constant-table coupling_gradient: both sum the same
    n products, each in its own order: within 2 gamma_{n + len + 1} of the sum of the magnitudes."""
    import wlsqm.hip as whip
    n = 300
    st = SR.planes_structure(n, 9, nop, seed=43)
    rows = SR.rows_of_structure(st)
    lens = np.array([len(r) for r in rows])
    A = SR.dense_planes(rows, n, nop)
    rng = np.random.default_rng([109, m, nop])
    cp = rng.standard_normal((m, m, nop))
    lam, x = rng.standard_normal((n, m)), rng.standard_normal((n, m))
    op = _operator(whip, st)
    point = whip.StencilSystemSolver(op, _t(PR.constant_table(cp, n)), diag=1.0)
    const = whip.StencilSystemSolver(op, cp, diag=1.0)
    got = point.coupling_gradient(_t(lam), _t(x))
    assert tuple(got.shape) == (m, m, nop, n) and got.is_contiguous()
    got = got.cpu().numpy()
    want, mag = PR.coupling_gradient_statement(A, lam, x)
    # numpy's own A_o x carries the roundings of its sum too: twice the chain
    bound = 2 * R.gamma(lens + 3)[None, None, None, :] * mag
    assert np.all(np.abs(got - want) <= bound), float((np.abs(got - want) / np.maximum(bound, 1e-300)).max())
    summed = const.coupling_gradient(_t(lam), _t(x)).cpu().numpy()
    room = 2 * float(R.gamma(n + lens.max() + 1)) * mag.sum(axis=-1)
    assert np.all(np.abs(got.sum(axis=-1) - summed) <= room)
    point.close(); const.close(); op.close()


def _norm_criterion(got, want, kappa, what):
    """Within kappa_2(M) rtol times the gradient's norm of the dense implicit-function gradient."""
    dist, bound = np.linalg.norm(got - want), kappa * KR.RTOL * np.linalg.norm(want)
    print("%s: distance %.3e, |gradient| %.3e, bound %.3e (at %.3g of it)" % (what, dist, np.linalg.norm(want), bound, dist / bound))
    assert dist <= bound, what


def test_autograd_reaches_b_diag_coupling_coefficients_and_the_point_table(wlsqm):
    """differentiable_stencil_system_solve on elasticity-2D-n130 with the heterogeneous table: every gradient against the dense
    implicit-function gradient of the library's own matrix, within kappa_2(M) rtol times the gradient's norm."""
    import torch
    import wlsqm.hip as whip
    name = "elasticity-2D-n130"
    made = _system(name)
    sy, op, A, M, kappa = made["sy"], made["op"], made["A"], made["M"], made["kappa"]
    n, mm, nop, cpt = sy["n"], sy["m"], sy["nop"], sy["coupling"]
    w = SA.adjoint_rhs(n, mm)
    D = np.zeros((mm, mm, n))
    G = PR.implicit_gradients(A, cpt, D, sy["b"], w)
    cap = 2 * max(PR.CAPS[name]["jacobi"], PR.TRANSPOSED_CAPS[name]["jacobi"])
    slots_now, own_now = op.coefficients()
    b, diag, slots, own = (t.clone().requires_grad_() for t in (_t(sy["b"]), _t(D), slots_now, own_now))
    coupling = _t(cpt).requires_grad_()
    solver = whip.StencilSystemSolver(op, _t(np.ones_like(cpt)), diag=diag)       # the table is written by the forward
    x = whip.differentiable_stencil_system_solve(solver, b, coefficients=(slots, own), coupling=coupling, rtol=KR.RTOL, maxiter=cap)
    assert x.requires_grad and tuple(x.shape) == (n, mm) and solver.info().status == 0
    assert solver.coupling.data_ptr() == coupling.data_ptr()
    solver.set_coupling(_t(np.zeros_like(cpt)))                          # the backward puts the table back where the forward had it
    (x * _t(w)).sum().backward()
    assert solver.coupling.data_ptr() == coupling.data_ptr()
    _norm_criterion(x.detach().cpu().numpy(), G["x"], kappa, "x")
    _norm_criterion(b.grad.cpu().numpy(), G["b"], kappa, "dL/db")
    _norm_criterion(diag.grad.cpu().numpy(), G["diag"], kappa, "dL/ddiag")
    assert tuple(coupling.grad.shape) == cpt.shape and coupling.grad.is_cuda
    _norm_criterion(coupling.grad.cpu().numpy(), G["coupling"], kappa, "dL/dcoupling")
    hoods, nk = sy["hoods"], sy["nk"]
    own_mask = op._own_mask.cpu().numpy() if op._own_mask is not None else np.zeros(n, bool)
    live = np.arange(hoods.shape[1])[None, :] < nk[:, None]
    cols = np.where(live, hoods, 0)
    want_s = np.where(live[None], np.take_along_axis(G["entries"], np.broadcast_to(cols[None], (nop,) + cols.shape), axis=2), 0.0)
    want_o = np.where(own_mask[None], G["entries"][:, np.arange(n), np.arange(n)], 0.0)
    gs, go = slots.grad.cpu().numpy(), own.grad.cpu().numpy()
    assert not gs[:, ~live].view(np.uint64).any() and not go[:, ~own_mask].view(np.uint64).any()
    _norm_criterion(np.concatenate([gs.reshape(-1), go.reshape(-1)]), np.concatenate([want_s.reshape(-1), want_o.reshape(-1)]), kappa,
                    "dL/dcoefficients")
    solver.close()
    # S: an operator of its own (the forward refits it), the table read as it is
    S = _t(sy["S"]).requires_grad_()
    op2 = whip.StencilOperator(sy["dim"], sy["order"], _t(sy["S"]), _t(sy["hoods"]), _t(sy["nk"]), _t(sy["knowns"]), _t(sy["wm"]), _t(sy["rows"]))
    solver2 = whip.StencilSystemSolver(op2, _t(cpt), diag=sy["diag"])
    x2 = whip.differentiable_stencil_system_solve(solver2, _t(sy["b"]), S=S, rtol=KR.RTOL, maxiter=cap)
    (x2 * _t(w)).sum().backward()
    assert tuple(S.grad.shape) == tuple(S.shape)
    _norm_criterion(S.grad.cpu().numpy(), PR.geometry_truth(sy, cpt, G["x"], G["lam"]), kappa, "dL/dS")
    solver2.close(); op2.close()
