"""GPU tests of the gradients through implicit solves (wlsqm.hip.differentiable_stencil_solve, StencilSolver.gradients and
solve(transpose=True), csrc/krylov.hip's krylov_grads_kernel).

  1. the grads kernel alone: `values` and `diag` bit for bit the two-rounding numpy statement (tests/_krylov_adjoint_ref.py), +0.0 in
     every padding position, `scale` against exact arithmetic within a derived bound, the same bits again and into given outputs;
  2. transposed solves held to the reference run on M^T by the criteria of tests/test_gpu_krylov.py; bit for bit the forward solve of
     an operator packed from the transposed rows; behind op.update the moved values;
  3. autograd on b, diag and the coefficients within the bilinear bounds of the two solves' distances from the dense solutions;
  4. autograd on the point table against the CPU geometry adjoint, within the reference solver's and the parent kernels' own shares;
  5. one operator shared by the steps of a loop; 6. refusals.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

import _krylov_adjoint_ref as KA
import _krylov_ref as KR
import _stencil_ref as R
from _device_helpers import bits, dev as _t, nan as _nan, same_bits as _same_bits, wlsqm  # noqa: F401 (fixture)
from test_gpu_krylov import _held_to_the_reference, _system

pytestmark = pytest.mark.gpu


def _from_structure(whip, st, n):
    return whip.StencilOperator.from_coefficients(_t(st["hoods"]), _t(st["nk"]), _t(st["slots"]), n, own=_t(st["own"]),
                                                  own_mask=_t(st["own_mask"]))


def _zeros(n):
    import torch
    return torch.zeros(n, dtype=torch.float64, device="cuda")


# ---- 1. the grads kernel alone --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nrows", (1, 63, 64, 65, 130, 300, 65537))
def test_grads_kernel_against_its_statement_and_exact_arithmetic(wlsqm, nrows):
    """values and diag: one product of two roundings each, so the numpy statement's bits.  scale = -(sum_j lam_j * rowsum_j): the row
    sum is an fma chain of len_j roundings (gamma_{len_j} sum |val x|), the product by lam_j one more, and the sum of the nrows lane
    products goes through the wave's tree, the workgroup's waves, the reduce kernel's loop, tree and waves as every dot product of
    tests/test_gpu_krylov.py does, at most nrows + depth roundings with depth = 6 + 3 + ceil(nwg / 256) + 6 + 3; the negation is
    exact.  In all gamma_{L + 1 + nrows + depth} sum_j |lam_j| sum_e |val x|, L the longest row."""
    import torch
    import wlsqm.hip as whip
    K, c = 9, -0.75
    st = KR.square_structure(nrows, K, seed=31)
    rows = R.rows_of(st["hoods"], st["nk"], st["slots"], st["own"], st["own_mask"], st["pts"])
    lens = np.array([len(r) for r in rows])
    if nrows >= 130:
        assert lens.min() == 0 and np.all(lens[64:128] == 0)            # empty rows and an empty slice
    m = R.pack(rows, 1)
    rng = np.random.default_rng([61, nrows])
    lam = rng.standard_normal(nrows) * 10.0 ** rng.integers(-2, 3, nrows)
    x = rng.standard_normal(nrows) * 10.0 ** rng.integers(-2, 3, nrows)
    d = rng.standard_normal(nrows)
    op = _from_structure(whip, st, nrows)
    assert np.array_equal(op._m["col"].cpu().numpy(), m["col"]) and _same_bits(op._val.cpu().numpy(), m["val"])
    total = op._m["total"]
    solver = whip.StencilSolver(op, diag=_t(d), scale=c)
    if nrows == 130:                                                     # behind a solve that has stopped: `done` is set and ignored
        assert solver.solve(_t(rng.standard_normal(nrows)), _zeros(nrows), maxiter=1).status >= 0
    lam_t, x_t = _t(lam), _t(x)
    got = solver.gradients(lam_t, x_t, values=True, diag=True, scale=True)
    assert whip.last_kernel() == "krylov-grads"
    assert tuple(got.values.shape) == (total,) and tuple(got.diag.shape) == (nrows,) and got.scale.dim() == 0 and got.scale.is_cuda
    want_values, want_diag = KA.grads_statement(m, nrows, c, lam, x)
    values = got.values.cpu().numpy()
    row, at = KA.entries_of(m, nrows)
    padding = np.ones(total, bool)
    padding[at] = False
    assert not values[padding].view(np.uint64).any()                     # +0.0, the lanes of rows beyond nrows included
    assert _same_bits(values, want_values)
    assert _same_bits(got.diag.cpu().numpy(), want_diag)
    exact, mag = KA.exact_triple(lam[row], m["val"][0][at], x[m["col"][at]])
    nwg = (nrows + 255) // 256
    depth = 6 + 3 + math.ceil(nwg / 256) + 6 + 3
    bound = float(R.gamma(int(lens.max()) + 1 + nrows + depth)) * float(mag)
    scale = float(got.scale)
    print("nrows %d: scale %.6e at %.3g of its bound" % (nrows, scale, float(abs(Fraction(scale) + exact) / Fraction(bound)) if bound else 0.0))
    assert abs(Fraction(scale) + exact) <= bound, (nrows, scale, float(exact), bound)
    # the same bits again, into outputs passed in (NaN before: every position is written), and from each output asked for alone
    outs = (_nan(total), _nan(nrows), _nan())
    again = solver.gradients(lam_t, x_t, values=outs[0], diag=outs[1], scale=outs[2])
    assert again.values is outs[0] and again.diag is outs[1] and again.scale is outs[2]
    alone = (solver.gradients(lam_t, x_t, values=True), solver.gradients(lam_t, x_t, diag=True), solver.gradients(lam_t, x_t, scale=True))
    assert alone[0].diag is None and alone[0].scale is None and alone[2].values is None
    for other in (again, whip.SolveGradients(alone[0].values, alone[1].diag, alone[2].scale)):
        for a, b in zip(other, got):
            assert torch.equal(bits(a), bits(b))
    # the row sums are the product's bits: with M = A (diag 0, scale 1) the product's dot0 = (A x, lam) goes through the same lane
    # products, tree and reduce, so scale is its negation bit for bit
    unit = whip.StencilSolver(op, diag=0.0, scale=1.0)
    _, dot_lam, _ = unit.product(x_t, lam_t)
    assert float(unit.gradients(lam_t, x_t, scale=True).scale) == -dot_lam
    unit.close(); solver.close(); op.close()


# ---- 2. transposed solves ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", KR.GPU_SYSTEMS)
def test_transposed_solve(wlsqm, name):
    m = _system(name)
    n, M = m["sy"]["n"], m["M"]
    g = KA.adjoint_rhs(n)
    mt = dict(sy=dict(b=g), M=M.T, xstar=np.linalg.solve(M.T, g), stop=KR.RTOL * np.linalg.norm(g), kappa=m["kappa"])
    lam = _zeros(n)
    cap = KA.transposed_maxiter(name)
    info = m["solver"].solve(_t(g), lam, rtol=KR.RTOL, maxiter=cap, transpose=True)
    _held_to_the_reference(mt, lam.cpu().numpy(), info, np.zeros(n), KR.jacobi(M.T), cap, name + " transposed")
    assert m["op"].fill_transposed is not None                           # built at the first transposed use


@pytest.mark.parametrize("name", ("random-n130", "random-n1000"))
def test_transposed_solve_is_the_solve_of_the_transposed_rows(wlsqm, name):
    import torch
    import wlsqm.hip as whip
    m = _system(name)
    sy, n = m["sy"], m["sy"]["n"]
    st = sy["st"]
    trows = R.transpose_rows(R.rows_of(st["hoods"], st["nk"], st["slots"], st["own"], st["own_mask"], st["pts"]), n)
    K2 = max(len(r) for r in trows)
    hoods, nk, slots = np.full((n, K2), -1, np.int32), np.zeros(n, np.int32), np.full((1, n, K2), np.nan)
    for i, r in enumerate(trows):
        nk[i] = len(r)
        for e, (col, v) in enumerate(r):
            hoods[i, e], slots[0, i, e] = col, v[0]
    top = whip.StencilOperator.from_coefficients(_t(hoods), _t(nk), _t(slots), n)
    tsolver = whip.StencilSolver(top, **m["args"])
    g = _t(KA.adjoint_rhs(n))
    cap = KA.transposed_maxiter(name)
    lam, want = _zeros(n), _zeros(n)
    info = m["solver"].solve(g, lam, maxiter=cap, transpose=True)
    info_t = tsolver.solve(g, want, maxiter=cap)
    assert info == info_t and info.status == 0 and torch.equal(bits(lam), bits(want))
    out, dot_w, dot_v = m["solver"].product(g, transpose=True)
    out_t, dot_w_t, dot_v_t = tsolver.product(g)
    assert torch.equal(bits(out), bits(out_t)) and (dot_w, dot_v) == (dot_w_t, dot_v_t)
    lam2 = _zeros(n)
    m["solver"].enqueue(g, lam2, cap, transpose=True)
    assert m["solver"].info() == info and torch.equal(bits(lam2), bits(lam))
    tsolver.close(); top.close()


def test_transposed_solve_behind_update_uses_the_moved_values(wlsqm):
    import torch
    import wlsqm.hip as whip
    name = "2D-tau0.25-n130"
    sy = KR.system(name)
    n = sy["n"]
    moved = sy["S"] + 0.05 * n ** -0.5 * np.random.default_rng(67).standard_normal(sy["S"].shape)
    build = lambda S: whip.StencilOperator(2, 2, _t(S), _t(sy["hoods"]), _t(sy["nk"]), _t(sy["knowns"]), _t(sy["wm"]), _t(sy["rows"]))
    op, fresh = build(sy["S"]), build(moved)
    solver, fresh_solver = (whip.StencilSolver(o, diag=sy["diag"], scale=sy["scale"]) for o in (op, fresh))
    g = _t(KA.adjoint_rhs(n))
    cap = 2 * KA.transposed_maxiter(name)
    at_start, behind, want = _zeros(n), _zeros(n), _zeros(n)
    assert solver.solve(g, at_start, maxiter=cap, transpose=True).status == 0          # builds the transposed matrix
    op.update(_t(moved))
    info = solver.solve(g, behind, maxiter=cap, transpose=True)
    assert info == fresh_solver.solve(g, want, maxiter=cap, transpose=True) and info.status == 0
    assert torch.equal(bits(behind), bits(want)) and not torch.equal(bits(behind), bits(at_start))
    for o in (solver, fresh_solver, op, fresh):
        o.close()


# ---- 3. autograd on b, diag and the coefficients -----------------------------------------------------------------------------------------

def _count_calls(monkeypatch, whip):
    """The list that the solver's solves and gradient launches and the two fit calls of the geometry gradient append their names to
    from now on (the backward pass runs on autograd's thread): what a pass launched, in order."""
    calls = []
    for owner, name in ((whip.StencilSolver, "solve"), (whip.StencilSolver, "gradients"), (whip, "fit_cloud_device"),
                        (whip, "fit_cloud_geometry_adjoint_device")):
        def wrap(*a, _real=getattr(owner, name), _name=name, **kw):
            calls.append(_name + ("-transposed" if kw.get("transpose") else ""))
            return _real(*a, **kw)
        monkeypatch.setattr(owner, name, wrap)
    return calls


def _dense_pair(M, b, w):
    return np.linalg.solve(M, b), np.linalg.solve(M.T, w)


def _within_the_solve_criterion(M, kappa, rhs, got, star, what):
    """The error criterion of the solves: the relative error within kappa_2 times the relative true residual.  Returns the distance."""
    e = np.linalg.norm(got - star)
    true = np.linalg.norm(rhs - M @ got)
    print("%s: distance %.3e, relative error %.3e, bound %.3e" % (what, e, e / np.linalg.norm(star), kappa * true / np.linalg.norm(rhs)))
    assert e / np.linalg.norm(star) <= kappa * true / np.linalg.norm(rhs) * (1 + 1e-6), what
    return e


@pytest.mark.parametrize("name", ("random-n130", "2D-tau0.25-n130", "2D-dirichlet-n130"))
def test_autograd_reaches_b_diag_and_coefficients(wlsqm, monkeypatch, name):
    """With e_x and e_lam the 2-norm distances of the device's x and lam from the dense solves (each held to the solves' criterion),
    |lam_j x_k - lam*_j x*_k| <= e_lam |x*_k| + |lam*_j| e_x + e_lam e_x, and each product carries two roundings: the bounds below."""
    import torch
    import wlsqm.hip as whip
    sy = KR.system(name)
    n, c = sy["n"], sy["scale"]
    if sy["kind"] == "random":                                           # two planes, the second the system's: the first gets zeros
        st = sy["st"]
        slots0 = np.concatenate([np.random.default_rng(71).standard_normal(st["slots"].shape), st["slots"]])
        own0 = np.concatenate([np.random.default_rng(73).standard_normal(st["own"].shape), st["own"]])
        op = whip.StencilOperator.from_coefficients(_t(st["hoods"]), _t(st["nk"]), _t(slots0), n, own=_t(own0), own_mask=_t(st["own_mask"]))
        o, hoods, nk, own_mask = 1, st["hoods"], st["nk"], st["own_mask"]
    else:
        op = whip.StencilOperator(sy["dim"], sy["order"], _t(sy["S"]), _t(sy["hoods"]), _t(sy["nk"]), _t(sy["knowns"]), _t(sy["wm"]), _t(sy["rows"]))
        o, hoods, nk, own_mask = 0, sy["hoods"], sy["nk"], np.ones(n, bool)
    d0 = KA.diag_vector(sy)
    M = np.diag(d0) + c * op.to_sparse_csr(o).to_dense().cpu().numpy()
    kappa = np.linalg.cond(M)
    w = KA.adjoint_rhs(n)
    xs, ls = _dense_pair(M, sy["b"], w)
    slots_now, own_now = op.coefficients()
    b, diag, slots, own = (t.clone().requires_grad_() for t in (_t(sy["b"]), _t(d0), slots_now, own_now))
    solver = whip.StencilSolver(op, o=o, diag=diag, scale=c)
    cap = 2 * max(KR.maxiter(name), KA.transposed_maxiter(name))
    calls = _count_calls(monkeypatch, whip)
    x = whip.differentiable_stencil_solve(solver, b, coefficients=(slots, own), maxiter=cap)
    assert x.requires_grad and solver.info().status == 0 and calls == ["solve"]
    del calls[:]
    (x * _t(w)).sum().backward()
    assert calls == ["solve-transposed", "gradients"]
    e_x = _within_the_solve_criterion(M, kappa, sy["b"], x.detach().cpu().numpy(), xs, name + " x")
    e_lam = _within_the_solve_criterion(M.T, kappa, w, b.grad.cpu().numpy(), ls, name + " lam")
    u2 = float(R.gamma(2))
    room = e_lam * np.abs(xs).max() + np.abs(ls).max() * e_x + e_lam * e_x + u2 * np.linalg.norm(ls * xs)
    dist = np.linalg.norm(diag.grad.cpu().numpy() + ls * xs)
    print("%s diag: distance %.3e, bound %.3e" % (name, dist, room))
    assert dist <= room
    # the entries: slot k of row j names column hoods[j, k], the own entry column j
    K = hoods.shape[1]
    live = np.arange(K)[None, :] < nk[:, None]
    cols = np.where(live, hoods, 0)
    per = lambda lj, xk: abs(c) * (e_lam * np.abs(xk) + np.abs(lj) * e_x + e_lam * e_x) + u2 * abs(c) * (np.abs(lj) + e_lam) * (np.abs(xk) + e_x)
    gs, go = slots.grad.cpu().numpy(), own.grad.cpu().numpy()
    want_s = np.where(live, -c * ls[:, None] * xs[cols], 0.0)
    want_o = np.where(own_mask, -c * ls * xs, 0.0)
    assert np.all(np.abs(gs[o] - want_s) <= np.where(live, per(ls[:, None], xs[cols]), 0.0))
    assert np.all(np.abs(go[o] - want_o) <= np.where(own_mask, per(ls, xs), 0.0))
    print("%s entries: worst distance %.3e" % (name, max(np.abs(gs[o] - want_s).max(), np.abs(go[o] - want_o).max())))
    for plane in range(op.nop):
        if plane != o:
            assert not gs[plane].view(np.uint64).any() and not go[plane].view(np.uint64).any()
    assert not gs[o][~live].view(np.uint64).any() and not go[o][~own_mask].view(np.uint64).any()
    # only what requires a gradient: b alone is the transposed solve and nothing else; nothing at all launches nothing
    b2 = _t(sy["b"]).requires_grad_()
    plain = whip.StencilSolver(op, o=o, diag=diag.detach(), scale=c)
    x2 = whip.differentiable_stencil_solve(plain, b2, coefficients=(slots.detach(), own.detach()), maxiter=cap)
    assert torch.equal(bits(x2.detach()), bits(x.detach()))
    del calls[:]
    (x2 * _t(w)).sum().backward()
    assert calls == ["solve-transposed"] and torch.equal(bits(b2.grad), bits(b.grad))
    del calls[:]
    x3 = whip.differentiable_stencil_solve(plain, _t(sy["b"]), maxiter=cap)
    assert not x3.requires_grad and calls == ["solve"] and torch.equal(bits(x3), bits(x.detach()))
    # diag alone, on the operator as it is (neither S nor coefficients): b gets None
    diag3 = _t(d0).requires_grad_()
    b3 = _t(sy["b"])
    x4 = whip.differentiable_stencil_solve(whip.StencilSolver(op, o=o, diag=diag3, scale=c), b3, maxiter=cap)
    del calls[:]
    (x4 * _t(w)).sum().backward()
    assert calls == ["solve-transposed", "gradients"] and b3.grad is None and torch.equal(bits(diag3.grad), bits(diag.grad))
    solver.close(); plain.close(); op.close()


# ---- 4. autograd on the point table --------------------------------------------------------------------------------------------------------

_shares = {}


def _geometry_case(name):
    """What the tests of dL/dS share about a system, computed once: the truth T from the dense solutions, the reference solver's own
    share a and the parent kernels' share b_dev, measured in this run."""
    if name in _shares:
        return _shares[name]
    import wlsqm.hip as whip
    m = _system(name)
    sy, M, n = m["sy"], m["M"], m["sy"]["n"]
    w = KA.adjoint_rhs(n)
    xs, ls = _dense_pair(M, sy["b"], w)
    T = KA.geometry_truth(sy, xs, ls)
    caps = 2 * KR.maxiter(name), 2 * KA.transposed_maxiter(name)
    xr, _, st_x, _ = KR.bicgstab_ref(M, sy["b"], np.zeros(n), KR.jacobi(M), KR.RTOL, 0.0, caps[0])
    lr, _, st_l, _ = KR.bicgstab_ref(M.T, w, np.zeros(n), KR.jacobi(M.T), KR.RTOL, 0.0, caps[1])
    assert st_x == st_l == KR.CONVERGED
    a = np.abs(KA.geometry_truth(sy, xr, lr) - T).max()
    # G: the geometry adjoint of the parent, called explicitly on the uploaded dense solutions
    t = {k: _t(sy[k]) for k in ("S", "hoods", "nk", "knowns", "wm")}
    rows = sy["rows"][0]
    no = rows.shape[-1]
    fi = np.zeros((n, no))
    fi[:, 0] = xs
    fi, F = _t(fi), _t(xs)
    g = _t(np.ascontiguousarray((-sy["scale"] * ls)[:, None] * np.broadcast_to(rows, (n, no))))
    whip.fit_cloud_device(sy["dim"], sy["order"], t["S"], F, t["hoods"], fi, t["nk"], t["knowns"], t["wm"])
    G = whip.fit_cloud_geometry_adjoint_device(sy["dim"], sy["order"], t["S"], F, t["hoods"], fi, t["nk"], t["knowns"], t["wm"], g)[0]
    b_dev = np.abs(G.cpu().numpy() - T).max()
    _shares[name] = dict(m=m, w=w, T=T, a=a, b_dev=b_dev, caps=caps)
    return _shares[name]


@pytest.mark.parametrize("name", ("2D-tau0.25-n130", "2D-dirichlet-n130", "3D-tau0.25-n1000"))
def test_autograd_reaches_the_point_table(wlsqm, monkeypatch, name):
    """|grad_S - T|_inf <= 8 a + 2 b_dev: T the CPU geometry adjoint fed the dense x*, lam*; a the distance from T of the same formula
    fed the reference solver's x, lam at the same rtol (8: the project's factor for a solver whose summation order differs); b_dev the
    distance from T of the parent's geometry adjoint on the uploaded x*, lam* (2: index_add_ sums in no fixed order)."""
    import torch
    import wlsqm.hip as whip
    case = _geometry_case(name)
    m, T = case["m"], case["T"]
    sy, n = m["sy"], m["sy"]["n"]
    S, b = _t(sy["S"]).requires_grad_(), _t(sy["b"])
    calls = _count_calls(monkeypatch, whip)
    x = whip.differentiable_stencil_solve(m["solver"], b, S=S, maxiter=max(case["caps"]))
    assert calls == ["solve"]
    del calls[:]
    (x * _t(case["w"])).sum().backward()
    assert calls == ["solve-transposed", "fit_cloud_device", "fit_cloud_geometry_adjoint_device"] and b.grad is None
    assert tuple(S.grad.shape) == tuple(S.shape)
    dist = np.abs(S.grad.cpu().numpy() - T).max()
    print("%s dL/dS: |T|_inf %.3e, a %.3e, b_dev %.3e, distance %.3e, bound %.3e"
          % (name, np.abs(T).max(), case["a"], case["b_dev"], dist, 8 * case["a"] + 2 * case["b_dev"]))
    assert dist <= 8 * case["a"] + 2 * case["b_dev"]


# ---- 5. one operator in a loop ---------------------------------------------------------------------------------------------------------------

def test_two_steps_share_one_operator(wlsqm):
    import torch
    import wlsqm.hip as whip
    name = "2D-tau0.25-n130"
    case = _geometry_case(name)
    sy = case["m"]["sy"]
    n = sy["n"]
    SA, SB = sy["S"], sy["S"] + 0.05 * n ** -0.5 * np.random.default_rng(79).standard_normal(sy["S"].shape)
    build = lambda S: whip.StencilOperator(2, 2, _t(S), _t(sy["hoods"]), _t(sy["nk"]), _t(sy["knowns"]), _t(sy["wm"]), _t(sy["rows"]))
    w = _t(case["w"])
    cap = max(case["caps"])

    def two_steps(solver1, solver2):
        S1, S2, b = _t(SA).requires_grad_(), _t(SB).requires_grad_(), _t(sy["b"]).requires_grad_()
        x1 = whip.differentiable_stencil_solve(solver1, b, S=S1, maxiter=cap)
        x2 = whip.differentiable_stencil_solve(solver2, x1, S=S2, maxiter=cap)
        (x2 * w).sum().backward()
        return x2.detach(), b.grad, S1.grad, S2.grad

    ops = [build(SB), build(SA), build(SB)]                              # the shared one starts at SB: the first step's update moves it
    solvers = [whip.StencilSolver(o, diag=sy["diag"], scale=sy["scale"]) for o in ops]
    shared = two_steps(solvers[0], solvers[0])
    apart = two_steps(solvers[1], solvers[2])
    assert torch.equal(bits(shared[0]), bits(apart[0])) and torch.equal(bits(shared[1]), bits(apart[1]))
    for got, want, what in ((shared[2], apart[2], "S1"), (shared[3], apart[3], "S2")):
        dist = float((got - want).abs().max())
        print("%s: shared against separate operators, distance %.3e, bound %.3e" % (what, dist, 2 * case["b_dev"]))
        assert dist <= 2 * case["b_dev"]
    assert float(shared[2].abs().max()) > 0 and float(shared[3].abs().max()) > 0
    for o in solvers + ops:
        o.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------

def test_refusals_on_the_device(wlsqm):
    import torch
    import wlsqm.hip as whip
    m = _system("2D-dirichlet-n130")
    solver, n = m["solver"], m["sy"]["n"]
    b = m["b"].clone().requires_grad_()
    with pytest.raises(RuntimeError, match="the forward solve did not converge: status 1, SolveInfo\\(status=1, iterations=1"):
        whip.differentiable_stencil_solve(solver, b, maxiter=1)
    # a forward that converges at once from the solution, an adjoint that cannot within the same single iteration
    x0 = _zeros(n)
    assert solver.solve(m["b"], x0, rtol=1e-12, maxiter=4 * KR.maxiter("2D-dirichlet-n130")).status == 0
    x = whip.differentiable_stencil_solve(solver, b, x0=x0, maxiter=1)
    assert solver.info().iterations == 0 and torch.equal(bits(x.detach()), bits(x0))
    with pytest.raises(RuntimeError, match="the adjoint solve did not converge: status 1"):
        (x * _t(KA.adjoint_rhs(n))).sum().backward()
    assert b.grad is None
    # inside a capture: the existing refusal
    refused = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="differentiable_stencil_solve reads the solve's scalars on the host and the stream is capturing"):
        with torch.cuda.graph(refused, stream=torch.cuda.Stream()):
            whip.differentiable_stencil_solve(solver, b)
    torch.cuda.synchronize()
    x = whip.differentiable_stencil_solve(solver, b, maxiter=4 * KR.maxiter("2D-dirichlet-n130"))       # the capture ended cleanly
    assert solver.info().status == 0
    with pytest.raises(ValueError, match="S and coefficients are two ways"):
        whip.differentiable_stencil_solve(solver, b, S=_t(m["sy"]["S"]), coefficients=m["op"].coefficients())
    same = whip.StencilOperator.from_coefficients(_t(m["sy"]["hoods"]), _t(m["sy"]["nk"]), m["op"].coefficients()[0], n)
    with pytest.raises(RuntimeError, match="made from coefficients: there is no fit to redo"):
        whip.differentiable_stencil_solve(whip.StencilSolver(same), b, S=_t(m["sy"]["S"]))
    with pytest.raises(ValueError, match="own goes together with an operator that has own entries"):
        whip.differentiable_stencil_solve(whip.StencilSolver(same), b, coefficients=m["op"].coefficients())
    same.close()
