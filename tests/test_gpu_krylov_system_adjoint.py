"""GPU tests of the gradients through coupled solves (wlsqm.hip.differentiable_stencil_system_solve, StencilSystemSolver.gradients,
coupling_gradient, set_coupling and solve(transpose=True), csrc/krylov.hip's krylov_system_grads_kernel).

  1. the gradient kernel alone: `values` and `diag` bit for bit the stated order of operations (tests/_krylov_system_adjoint_ref.py),
     +0.0 in every padding position, the same bits into given outputs and from each output alone, an unasked buffer untouched;
  2. transposed solves by section 17's criteria against the dense M^T of the library's own matrix(), within the caps; bit for bit the
     forward solve of an operator packed from the transposed rows with (a, b) exchanged in coupling and diag; the transposed product
     within section 24's bound; a diag tensor changed in place; the forward solve's bits afterwards; the refusal inside a capture;
  3. autograd on b, diag, the entries of every plane and coupling within the bilinear bounds of the two solves' distances from the
     dense solutions; on the point table against the CPU geometry adjoint within the reference solver's and the parent kernels' own
     shares; structure (None, exact zeros, no launch); two chained steps on one operator and solver; the failure paths.
"""
import numpy as np
import pytest

import _krylov_ref as KR
import _krylov_system_adjoint_ref as SA
import _krylov_system_ref as SR
import _stencil_ref as R
from _device_helpers import bits, dev as _t, nan as _nan, same_bits as _same_bits, wlsqm  # noqa: F401 (fixture)
from test_gpu_krylov_adjoint import _within_the_solve_criterion
from test_gpu_krylov_system import _held_to_the_reference, _operator, _solver, _system

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257, 300, 65537)
KERNEL_CASES = [(n, m, nop) for n in SIZES for m in (1, 2, 3, 4) for nop in (1, 3, 4, 7)]


def _zeros(n, m):
    import torch
    return torch.zeros((n, m), dtype=torch.float64, device="cuda")


# ---- 1. the gradient kernel alone ------------------------------------------------------------------------------------------------------

_structures = {}


def _structure(whip, nrows, nop):
    """The operator of planes_structure(nrows, 9, nop) and its SELL-64 arrays on the host, made once per (nrows, nop)."""
    if (nrows, nop) not in _structures:
        st = SR.planes_structure(nrows, 9, nop, seed=31)
        op = _operator(whip, st)
        sell = {k: op._m[k].cpu().numpy() for k in ("len", "width", "soff", "col")}
        lens = sell["len"].astype(np.int64)
        if nrows <= 300:                                                 # the layout is the reference's own packing
            rows = SR.rows_of_structure(st)
            ref = R.pack(rows, nop)
            assert np.array_equal(sell["col"], ref["col"]) and np.array_equal(sell["soff"], ref["soff"]) and np.array_equal(lens, ref["len"])
            assert nrows < 10 or any(len({c for c, _ in r}) < len(r) for r in rows)         # a column named twice
            assert nrows < 10 or any(any(c == i for c, _ in r) for i, r in enumerate(rows))  # own entries
        if nrows >= 130:
            assert lens.min() == 0 and np.all(lens[64:128] == 0)        # empty rows and an empty slice
        if nrows > 1:
            assert lens.min() < lens.max()                               # ragged rows
        _structures[nrows, nop] = (op, sell)
    return _structures[nrows, nop]


@pytest.mark.parametrize("nrows,m,nop", KERNEL_CASES)
def test_grads_kernel_bit_for_bit_its_statement(wlsqm, nrows, m, nop):
    import torch
    import wlsqm.hip as whip
    op, sell = _structure(whip, nrows, nop)
    total = op._m["total"]
    rng = np.random.default_rng([83, nrows, m, nop])
    coupling = rng.standard_normal((m, m, nop))
    lam = rng.standard_normal((nrows, m)) * 10.0 ** rng.integers(-2, 3, (nrows, m))
    x = rng.standard_normal((nrows, m)) * 10.0 ** rng.integers(-2, 3, (nrows, m))
    form = (nrows + m + nop) % 3                                         # the solver's diag takes no part: every form gives the same bits
    held = (0.75, rng.standard_normal((m, m)), _t(rng.standard_normal((m, m, nrows))))[form]
    solver = whip.StencilSystemSolver(op, coupling, diag=held)
    lam_t, x_t = _t(lam), _t(x)
    val_before = op._val.clone()
    got = solver.gradients(lam_t, x_t, values=True, diag=True)
    assert whip.last_kernel() == "krylov-system-grads"
    assert tuple(got.values.shape) == (nop, total) and tuple(got.diag.shape) == (m, m, nrows)
    values, diag = got.values.cpu().numpy(), got.diag.cpu().numpy()
    # the padding: +0.0 with its sign, in every plane, the lanes of rows beyond nrows included
    row, at_all = SA.entries_of(sell, nrows)
    padding = np.ones(total, bool)
    padding[at_all] = False
    assert 64 * int(sell["width"].astype(np.int64).sum()) == total and (nrows in (1, 64) or padding.any())
    assert not values[:, padding].view(np.uint64).any()
    # the bits: every row up to 300 points; above, the first and the last slice and sampled rows
    check = None if nrows <= 300 else np.unique(np.r_[0:64, rng.integers(64, nrows - 1, 40), 64 * ((nrows - 1) // 64):nrows])
    at, want_values, want_diag = SA.grads_statement(sell, nrows, coupling, lam, x, check)
    assert len(at) > 0 or nrows == 1
    assert _same_bits(values[:, at], want_values)
    assert _same_bits(diag if check is None else diag[:, :, check], want_diag)
    if check is not None:        # everywhere else the dense formula: the chains' 2 m roundings, and numpy's m^2 products of two and their sum
        c = sell["col"][at_all]
        U = np.einsum("abo,ja->jbo", coupling, lam)
        dense = -np.einsum("jbo,jb->oj", U[row], x[c])
        mag = np.einsum("abo,ja,jb->oj", np.abs(coupling), np.abs(lam[row]), np.abs(x[c]))
        assert np.all(np.abs(values[:, at_all] - dense) <= float(R.gamma(2 * m) + R.gamma(m * m + 2)) * mag)
        assert _same_bits(diag, -np.einsum("ia,ib->abi", lam, x))
    # the same bits into outputs passed in (NaN before: every position is written), and from each output asked for alone
    outs = (_nan(nop, total), _nan(m, m, nrows))
    before = torch.cuda.memory_allocated()
    again = solver.gradients(lam_t, x_t, values=outs[0], diag=outs[1])
    assert torch.cuda.memory_allocated() == before
    assert again.values is outs[0] and again.diag is outs[1]
    alone = (solver.gradients(lam_t, x_t, values=True), solver.gradients(lam_t, x_t, diag=True))
    assert alone[0].diag is None and alone[1].values is None
    for other in (again, whip.SystemGradients(alone[0].values, alone[1].diag)):
        for a, b in zip(other, got):
            assert torch.equal(bits(a), bits(b))
    # a pass without `values` stores into no plane: the poisoned buffer of the last call but one stays poisoned
    outs[0].fill_(float("nan"))
    only = solver.gradients(lam_t, x_t, diag=outs[1])
    assert only.values is None and bool(torch.isnan(outs[0]).all()) and torch.equal(bits(only.diag), bits(got.diag))
    assert torch.equal(bits(op._val), bits(val_before))                  # the operator's values are not an output
    solver.close()


# ---- 2. transposed solves -------------------------------------------------------------------------------------------------------------------

_transposed = {}


def _transposed_twin(m):
    """A StencilOperator packed from the transposed rows of the system's operator (the library's own planes), and the (a, b)-exchanged
    coupling and diag: the system whose forward solve is the transposed solve.  Made once per system."""
    import wlsqm.hip as whip
    name = m["name"]
    if name not in _transposed:
        sy, op = m["sy"], m["op"]
        n, nop = sy["n"], sy["nop"]
        slots, own = (t.cpu().numpy() for t in op.coefficients())
        if sy["kind"] == "random":
            hoods, nk, own_mask = sy["st"]["hoods"], sy["st"]["nk"], sy["st"]["own_mask"]
        else:
            hoods, nk, own_mask = sy["hoods"], sy["nk"], op._own_mask.cpu().numpy() if op._own_mask is not None else np.zeros(n, bool)
        rows = R.rows_of(hoods, nk, slots, own, own_mask, np.arange(n))
        th, tnk, tslots = SA.transposed_structure(rows, n, nop)
        top = whip.StencilOperator.from_coefficients(_t(th), _t(tnk), _t(tslots), n)
        d = sy["diag"]
        tdiag = _t(SA.transposed_diag(d)) if np.ndim(d) == 3 else SA.transposed_diag(d)
        _transposed[name] = dict(op=top, rows=R.rows_of(th, tnk, tslots), coupling=np.ascontiguousarray(np.transpose(sy["coupling"], (1, 0, 2))),
                                 diag=tdiag, solvers={})
    return _transposed[name]


def _named(name):
    m = _system(name)
    m["name"] = name
    return m


@pytest.mark.parametrize("name,pc", SA.GPU_CASES)
def test_transposed_solve(wlsqm, name, pc):
    import torch
    import wlsqm.hip as whip
    m = _named(name)
    sy, solver = m["sy"], _solver(m, pc)
    n, mm = sy["n"], sy["m"]
    g = SA.adjoint_rhs(n, mm)
    Mt = np.ascontiguousarray(solver.matrix().to_dense().cpu().numpy().T)
    mt = dict(M=Mt, bflat=g.reshape(-1), xstar=np.linalg.solve(Mt, g.reshape(-1)), stop=KR.RTOL * np.linalg.norm(g), kappa=m["kappa"])
    cap = SA.TRANSPOSED_CAPS[name][pc]
    # the forward solve before, for the bits it must keep
    fcap = SR.CAPS[name][pc]
    x_before = _zeros(n, mm)
    info_before = solver.solve(m["b"], x_before, maxiter=fcap)
    used = solver.memory_used()
    lam = _zeros(n, mm)
    info = solver.solve(_t(g), lam, rtol=KR.RTOL, maxiter=cap, transpose=True)
    assert solver.x is lam and m["op"].fill_transposed is not None       # built at the first transposed use
    _held_to_the_reference(mt, lam.cpu().numpy().reshape(-1), info, None, pc, cap, "%s %s transposed" % (name, pc))
    # bit for bit the forward solve of the operator packed from the transposed rows
    tw = _transposed_twin(m)
    if pc not in tw["solvers"]:
        tw["solvers"][pc] = whip.StencilSystemSolver(tw["op"], tw["coupling"], diag=tw["diag"], preconditioner=pc)
    want = _zeros(n, mm)
    info_t = tw["solvers"][pc].solve(_t(g), want, rtol=KR.RTOL, maxiter=cap)
    assert info == info_t and torch.equal(bits(lam), bits(want))
    out, dot_w, dot_v = solver.product(_t(g), transpose=True)
    out_t, dot_w_t, dot_v_t = tw["solvers"][pc].product(_t(g))
    assert torch.equal(bits(out), bits(out_t)) and (dot_w, dot_v) == (dot_w_t, dot_v_t)
    lam2, gt = _zeros(n, mm), _t(g)
    before = torch.cuda.memory_allocated()
    solver.enqueue(gt, lam2, cap, rtol=KR.RTOL, transpose=True)          # the transposed matrix exists: launches only
    assert torch.cuda.memory_allocated() == before
    assert solver.info() == info and torch.equal(bits(lam2), bits(lam))
    # a forward solve after a transposed one keeps the bits it had before, in the same workspace
    x_after = _zeros(n, mm)
    assert solver.solve(m["b"], x_after, maxiter=fcap) == info_before and torch.equal(bits(x_after), bits(x_before))
    assert solver.memory_used() == used


@pytest.mark.parametrize("name", SA.AUTOGRAD_SYSTEMS)
def test_transposed_product_within_the_products_bound(wlsqm, name):
    """Section 24's bound on the transposed rows: an unknown of T = m nop len + m terms within gamma_{T + 2} of the sum of their
    magnitudes, against exact arithmetic and against matrix().T @ v."""
    m = _named(name)
    sy, solver = m["sy"], _solver(m, "jacobi")
    n, mm, nop = sy["n"], sy["m"], sy["nop"]
    tw = _transposed_twin(m)
    v = np.random.default_rng([89, n]).standard_normal((n, mm))
    got = solver.product(_t(v), transpose=True)[0].cpu().numpy()
    exact, mag = SR.exact_product(tw["rows"], tw["coupling"], SA.transposed_diag(sy["diag"]), v)
    lens = np.array([len(r) for r in tw["rows"]])
    bound = R.gamma(mm * nop * lens + mm + 2)[:, None] * mag
    err = np.abs(got - exact)
    print("%s: transposed product at %.3f of its bound" % (name, float((err / np.maximum(bound, 1e-300)).max())))
    assert np.all(err <= bound)
    dense = (solver.matrix().to_dense().cpu().numpy().T @ v.reshape(-1)).reshape(n, mm)
    print("%s: against matrix().T @ v at %.3f of the bound" % (name, float((np.abs(got - dense) / np.maximum(bound, 1e-300)).max())))
    assert np.all(np.abs(got - dense) <= bound)


def test_a_changed_diag_tensor_is_seen_by_the_next_transposed_solve(wlsqm):
    import torch
    import wlsqm.hip as whip
    m = _named("random-m2")
    sy = m["sy"]
    n, mm = sy["n"], sy["m"]
    cap = SA.TRANSPOSED_CAPS["random-m2"]["jacobi"]
    diag = _t(sy["diag"])
    solver = whip.StencilSystemSolver(m["op"], sy["coupling"], diag=diag)
    g = _t(SA.adjoint_rhs(n, mm))
    l1, l2, l3 = _zeros(n, mm), _zeros(n, mm), _zeros(n, mm)
    first = solver.solve(g, l1, maxiter=cap, transpose=True)
    diag.mul_(1.5)                                                       # read in place, with its indices exchanged: no transposed copy
    second = solver.solve(g, l2, maxiter=cap, transpose=True)
    fresh = whip.StencilSystemSolver(m["op"], sy["coupling"], diag=_t(1.5 * sy["diag"]))
    third = fresh.solve(g, l3, maxiter=cap, transpose=True)
    assert first.status == second.status == 0 and second == third
    assert torch.equal(bits(l2), bits(l3)) and not torch.equal(bits(l1), bits(l2))
    Mt = fresh.matrix().to_dense().cpu().numpy().T
    gf = g.cpu().numpy().reshape(-1)
    assert np.linalg.norm(gf - Mt @ l2.cpu().numpy().reshape(-1)) <= 2 * KR.RTOL * np.linalg.norm(gf)
    # set_coupling: the next solve reads the new table, and a solver built with it gives the same bits
    cp2 = 0.5 * sy["coupling"]
    assert solver.set_coupling(cp2) is solver
    l4, l5 = _zeros(n, mm), _zeros(n, mm)
    swept = solver.solve(g, l4, maxiter=cap, transpose=True)
    built = whip.StencilSystemSolver(m["op"], cp2, diag=diag)
    assert swept == built.solve(g, l5, maxiter=cap, transpose=True) and swept.status == 0
    assert torch.equal(bits(l4), bits(l5)) and not torch.equal(bits(l4), bits(l2))
    solver.close(); fresh.close(); built.close()


def test_prepare_transpose_inside_a_capture_raises(wlsqm):
    import torch
    import wlsqm.hip as whip
    sy = SR.system("random-m2")
    n, mm = sy["n"], sy["m"]
    op = _operator(whip, sy["st"])
    solver = whip.StencilSystemSolver(op, sy["coupling"], diag=_t(sy["diag"]))
    g, lam = _t(SA.adjoint_rhs(n, mm)), _zeros(n, mm)
    refused = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="no transposed matrix yet and the stream is capturing: call prepare_transpose before the capture"):
        with torch.cuda.graph(refused, stream=torch.cuda.Stream()):
            solver.prepare_transpose()
    torch.cuda.synchronize()
    assert op.fill_transposed is None
    assert solver.prepare_transpose() is True and solver.prepare_transpose() is False and op.fill_transposed is not None
    assert solver.solve(g, lam, maxiter=SA.TRANSPOSED_CAPS["random-m2"]["jacobi"], transpose=True).status == 0
    # set_coefficients keeps the transposed values refreshed, as the operator does for every user of them
    slots, own = op.coefficients()
    op.set_coefficients(0.5 * slots, 0.5 * own)                          # halved: the system stays diagonally dominant
    fresh_op = whip.StencilOperator.from_coefficients(_t(sy["st"]["hoods"]), _t(sy["st"]["nk"]), 0.5 * slots, n, own=0.5 * own,
                                                      own_mask=_t(sy["st"]["own_mask"]))
    fresh = whip.StencilSystemSolver(fresh_op, sy["coupling"], diag=_t(sy["diag"]))
    l1, l2 = _zeros(n, mm), _zeros(n, mm)
    assert solver.solve(g, l1, maxiter=400, transpose=True) == fresh.solve(g, l2, maxiter=400, transpose=True)
    assert torch.equal(bits(l1), bits(l2)) and not torch.equal(bits(l1), bits(lam))
    solver.close(); fresh.close(); op.close(); fresh_op.close()


# ---- 3. autograd --------------------------------------------------------------------------------------------------------------------------

def _count_calls(monkeypatch, whip):
    """The list that the solver's solves and gradient launches and the two fit calls of the geometry gradient append their names to
    from now on (the backward pass runs on autograd's thread): what a pass launched, in order."""
    calls = []
    S = whip.StencilSystemSolver
    for owner, name in ((S, "solve"), (S, "gradients"), (S, "coupling_gradient"), (whip, "fit_cloud_device"),
                        (whip, "fit_cloud_geometry_adjoint_device")):
        def wrap(*a, _real=getattr(owner, name), _name=name, **kw):
            calls.append(_name + ("-transposed" if kw.get("transpose") else ""))
            return _real(*a, **kw)
        monkeypatch.setattr(owner, name, wrap)
    return calls


_cases = {}


def _case(name):
    """What the autograd tests share about a system, computed once and left unchanged: the operator, a diag tensor, the dense M of the
    library's own matrix(), the loss's w, the dense x* and lam*, kappa, the caps."""
    if name not in _cases:
        import wlsqm.hip as whip
        m = _named(name)
        sy, op = m["sy"], m["op"]
        n, mm = sy["n"], sy["m"]
        D = SR.diag_blocks(sy["diag"], mm, n)
        probe = whip.StencilSystemSolver(op, sy["coupling"], diag=_t(D))
        M = probe.matrix().to_dense().cpu().numpy()
        probe.close()
        w = SA.adjoint_rhs(n, mm)
        xs = np.linalg.solve(M, sy["b"].reshape(-1)).reshape(n, mm)
        ls = np.linalg.solve(M.T, w.reshape(-1)).reshape(n, mm)
        cap = 2 * max(SR.CAPS[name]["jacobi"], SA.TRANSPOSED_CAPS[name]["jacobi"])
        _cases[name] = dict(m=m, sy=sy, op=op, D=D, M=M, w=w, xs=xs, ls=ls, kappa=np.linalg.cond(M), cap=cap)
    return _cases[name]


def _bilinear(absc, L, X, e_lam, e_x, k, spec):
    """The bound of a computed sum_t c_t lam_t x_t against the same sum of the dense lam*, x*: with e_lam and e_x the 2-norm distances
    of the device's lam and x from them (which bound every component's), sum_t |c_t| (e_lam |x*_t| + |lam*_t| e_x + e_lam e_x), and
    gamma_k times the sum of the magnitudes of the computed terms, sum_t |c_t| (|lam*_t| + e_lam) (|x*_t| + e_x), for the k roundings
    of the stated chain.  `spec`: the einsum of (|c|, |lam*|, |x*|) that forms the sum over t."""
    ones_L, ones_X = np.ones_like(L), np.ones_like(X)
    s = lambda l, x: np.einsum(spec, absc, l, x)
    return (e_lam * s(ones_L, X) + e_x * s(L, ones_X) + e_lam * e_x * s(ones_L, ones_X)
            + float(R.gamma(k)) * s(L + e_lam, X + e_x))


@pytest.mark.parametrize("name,where", [("elasticity-2D-n130", "cpu"), ("reaction-2D-n130", "cuda"), ("random-m3", "cuda")])
def test_autograd_reaches_b_diag_entries_and_coupling(wlsqm, monkeypatch, name, where):
    import torch
    import wlsqm.hip as whip
    c = _case(name)
    sy, op, M, w, xs, ls = c["sy"], c["op"], c["M"], c["w"], c["xs"], c["ls"]
    n, mm, nop, cp = sy["n"], sy["m"], sy["nop"], sy["coupling"]
    if sy["kind"] == "random":
        hoods, nk, own_mask = sy["st"]["hoods"], sy["st"]["nk"], sy["st"]["own_mask"]
    else:
        hoods, nk, own_mask = sy["hoods"], sy["nk"], op._own_mask.cpu().numpy() if op._own_mask is not None else np.zeros(n, bool)
    slots_now, own_now = op.coefficients()
    b, diag, slots, own = (t.clone().requires_grad_() for t in (_t(sy["b"]), _t(c["D"]), slots_now, own_now))
    coupling = torch.from_numpy(cp.copy()).to(where).requires_grad_()
    solver = whip.StencilSystemSolver(op, np.zeros_like(cp) + 1.0, diag=diag)     # the table is written by the forward
    calls = _count_calls(monkeypatch, whip)
    x = whip.differentiable_stencil_system_solve(solver, b, coefficients=(slots, own), coupling=coupling, maxiter=c["cap"])
    assert x.requires_grad and tuple(x.shape) == (n, mm) and solver.info().status == 0 and calls == ["solve"]
    assert np.array_equal(solver.coupling, cp)
    solver.set_coupling(np.zeros_like(cp))                               # the backward puts the table back where the forward had it
    del calls[:]
    (x * _t(w)).sum().backward()
    assert calls == ["solve-transposed", "gradients", "coupling_gradient"] and np.array_equal(solver.coupling, cp)
    e_x = _within_the_solve_criterion(M, c["kappa"], sy["b"].reshape(-1), x.detach().cpu().numpy().reshape(-1), xs.reshape(-1), name + " x")
    e_lam = _within_the_solve_criterion(M.T, c["kappa"], w.reshape(-1), b.grad.cpu().numpy().reshape(-1), ls.reshape(-1), name + " lam")
    # diag (m, m, n): one term, one rounding
    dist = np.abs(diag.grad.cpu().numpy() + np.einsum("ia,ib->abi", ls, xs))
    room = _bilinear(np.ones(()), np.abs(ls), np.abs(xs), e_lam, e_x, 1, ",ia,ib->abi")
    print("%s diag: worst distance %.3e, at %.3g of its bound" % (name, dist.max(), (dist / room).max()))
    assert np.all(dist <= room)
    # every entry of every plane: slot k of row j names column hoods[j, k], the own entry column j; m^2 terms, 2 m roundings
    K = hoods.shape[1]
    live = np.arange(K)[None, :] < nk[:, None]
    cols = np.where(live, hoods, 0)
    absc = np.abs(cp)
    gs, go = slots.grad.cpu().numpy(), own.grad.cpu().numpy()
    assert gs.shape == tuple(slots.shape) and go.shape == tuple(own.shape)
    want_s = np.where(live[None], -np.einsum("abo,ja,jkb->ojk", cp, ls, xs[cols]), 0.0)
    want_o = np.where(own_mask[None], -np.einsum("abo,ja,jb->oj", cp, ls, xs), 0.0)
    room_s = np.where(live[None], _bilinear(absc, np.abs(ls), np.abs(xs[cols]), e_lam, e_x, 2 * mm, "abo,ja,jkb->ojk"), 0.0)
    room_o = np.where(own_mask[None], _bilinear(absc, np.abs(ls), np.abs(xs), e_lam, e_x, 2 * mm, "abo,ja,jb->oj"), 0.0)
    print("%s entries: worst distance %.3e, at %.3g of its bound" % (name, max(np.abs(gs - want_s).max(), np.abs(go - want_o).max()),
          max((np.abs(gs - want_s) / np.maximum(room_s, 1e-300)).max(), (np.abs(go - want_o) / np.maximum(room_o, 1e-300)).max())))
    assert np.all(np.abs(gs - want_s) <= room_s) and np.all(np.abs(go - want_o) <= room_o)
    assert not gs[:, ~live].view(np.uint64).any() and not go[:, ~own_mask].view(np.uint64).any()
    # coupling (m, m, nop), on the tensor's own device: lam_a^T A_o x_b, the bilinear bound summed over the points in the 2-norm, and
    # the roundings of the stacked product (a row's fma chain), of the products by lam and of their sum over n points
    assert coupling.grad.device.type == where and tuple(coupling.grad.shape) == cp.shape
    src, row = op._entries()
    col = op._m["col"][src].long()
    A = np.stack([torch.sparse_coo_tensor(torch.stack([row, col]), op._val[o, src], (n, n)).to_dense().cpu().numpy() for o in range(nop)])
    absA = np.stack([torch.sparse_coo_tensor(torch.stack([row, col]), op._val[o, src].abs(), (n, n)).to_dense().cpu().numpy() for o in range(nop)])
    want_c = -np.einsum("ia,oij,jb->abo", ls, A, xs)
    Ax = np.linalg.norm(np.einsum("oij,jb->obi", A, xs), axis=2)         # (nop, m): ||A_o x*_b||
    Atl = np.linalg.norm(np.einsum("oij,ia->oaj", A, ls), axis=2)        # (nop, m): ||A_o^T lam*_a||
    A2 = np.array([np.linalg.norm(A[o], 2) for o in range(nop)])
    longest = int(op._m["len"].max())
    room_c = (e_lam * Ax.T[None, :, :] + e_x * Atl.T[:, None, :] + e_lam * e_x * A2[None, None, :]
              + float(R.gamma(longest + n + 1)) * np.einsum("ia,oij,jb->abo", np.abs(ls) + e_lam, absA, np.abs(xs) + e_x))
    dist_c = np.abs(coupling.grad.cpu().numpy() - want_c)
    print("%s coupling: worst distance %.3e, at %.3g of its bound" % (name, dist_c.max(), (dist_c / room_c).max()))
    assert np.all(dist_c <= room_c)
    # only what requires a gradient: b alone is the transposed solve and nothing else
    b2 = _t(sy["b"]).requires_grad_()
    plain = whip.StencilSystemSolver(op, cp, diag=diag.detach())
    x2 = whip.differentiable_stencil_system_solve(plain, b2, coefficients=(slots.detach(), own.detach()), coupling=coupling.detach(),
                                                  maxiter=c["cap"])
    assert torch.equal(bits(x2.detach()), bits(x.detach()))
    del calls[:]
    (x2 * _t(w)).sum().backward()
    assert calls == ["solve-transposed"] and torch.equal(bits(b2.grad), bits(b.grad))
    # nothing requires one: no grad_fn; and an x0 that does, which receives none: the backward launches nothing
    del calls[:]
    x3 = whip.differentiable_stencil_system_solve(plain, _t(sy["b"]), maxiter=c["cap"])
    assert not x3.requires_grad and calls == ["solve"] and torch.equal(bits(x3), bits(x.detach()))
    x0 = _zeros(n, mm).requires_grad_()
    x4 = whip.differentiable_stencil_system_solve(plain, _t(sy["b"]), x0=x0, maxiter=c["cap"])
    marker = _t(np.zeros(n))
    op.apply(marker)
    last = whip.last_kernel()
    del calls[:]
    (x4 * _t(w)).sum().backward()
    assert calls == [] and whip.last_kernel() == last and x0.grad is None
    # diag alone, on the operator and the table as they are: b and coupling get None
    diag3 = _t(c["D"]).requires_grad_()
    b3 = _t(sy["b"])
    x5 = whip.differentiable_stencil_system_solve(whip.StencilSystemSolver(op, cp, diag=diag3), b3, maxiter=c["cap"])
    del calls[:]
    (x5 * _t(w)).sum().backward()
    assert calls == ["solve-transposed", "gradients"] and b3.grad is None and torch.equal(bits(diag3.grad), bits(diag.grad))
    solver.close(); plain.close()


def test_a_plane_without_coupling_gets_exact_zeros(wlsqm):
    import torch
    import wlsqm.hip as whip
    c = _case("random-m3")
    sy, op = c["sy"], c["op"]
    cp = sy["coupling"].copy()
    cp[:, :, 2] = 0.0                                                    # the system stays diagonally dominant
    slots_now, own_now = op.coefficients()
    slots, own = slots_now.clone().requires_grad_(), own_now.clone().requires_grad_()
    coupling = torch.from_numpy(cp).requires_grad_()
    solver = whip.StencilSystemSolver(op, sy["coupling"], diag=_t(c["D"]))
    x = whip.differentiable_stencil_system_solve(solver, _t(sy["b"]), coefficients=(slots, own), coupling=coupling, maxiter=4 * c["cap"])
    (x * _t(c["w"])).sum().backward()
    gs, go = slots.grad.cpu().numpy(), own.grad.cpu().numpy()
    assert np.all(gs[2] == 0.0) and np.all(go[2] == 0.0)
    for o in (0, 1, 3):
        assert np.abs(gs[o]).max() > 0.0
    assert np.abs(coupling.grad.numpy()[:, :, 2]).max() > 0.0            # the loss does depend on the table's entries of that plane
    solver.close()


_shares = {}


def _geometry_case(name):
    """What the tests of dL/dS share about a fitted system, computed once: the truth T from the dense solutions, the reference solver's
    own share a and the parent kernels' share b_dev, measured in this run."""
    if name in _shares:
        return _shares[name]
    import wlsqm.hip as whip
    c = _case(name)
    sy, M, w, xs, ls = c["sy"], c["M"], c["w"], c["xs"], c["ls"]
    n, mm, cp = sy["n"], sy["m"], sy["coupling"]
    T = SA.geometry_truth(sy, xs, ls)
    xr, _, st_x, _ = SR.solve_ref(M, sy["b"].reshape(-1), "jacobi", cap=c["cap"])
    lr, _, st_l, _ = SR.solve_ref(np.ascontiguousarray(M.T), w.reshape(-1), "jacobi", cap=c["cap"])
    assert st_x == st_l == KR.CONVERGED
    a = np.abs(SA.geometry_truth(sy, xr.reshape(n, mm), lr.reshape(n, mm)) - T).max()
    # G: the geometry adjoint of the parent, called explicitly on the uploaded dense solutions, per component, summed
    t = {k: _t(sy[k]) for k in ("S", "hoods", "nk", "knowns", "wm")}
    rows = sy["rows"]
    no = rows.shape[-1]
    per_case = np.broadcast_to(rows if rows.ndim == 3 else rows[:, None, :], (rows.shape[0], n, no))
    G = np.zeros_like(sy["S"])
    for b in range(mm):
        fi = np.zeros((n, no))
        fi[:, 0] = xs[:, b]
        fi, F = _t(fi), _t(np.ascontiguousarray(xs[:, b]))
        g = _t(np.ascontiguousarray(-np.einsum("jo,ojn->jn", ls @ cp[:, b, :], per_case)))
        whip.fit_cloud_device(sy["dim"], sy["order"], t["S"], F, t["hoods"], fi, t["nk"], t["knowns"], t["wm"])
        G += whip.fit_cloud_geometry_adjoint_device(sy["dim"], sy["order"], t["S"], F, t["hoods"], fi, t["nk"], t["knowns"], t["wm"], g)[0].cpu().numpy()
    b_dev = np.abs(G - T).max()
    _shares[name] = dict(c=c, T=T, a=a, b_dev=b_dev)
    return _shares[name]


@pytest.mark.parametrize("name", ("elasticity-2D-n130", "reaction-2D-n130"))
def test_autograd_reaches_the_point_table(wlsqm, monkeypatch, name):
    """|grad_S - T|_inf <= 8 a + 2 b_dev (DESIGN.md section 18's bound): T the CPU geometry adjoint fed the dense x*, lam*; a the
    distance from T of the same formula fed the reference solver's x, lam at the same rtol; b_dev the distance from T of the parent's
    geometry adjoint on the uploaded x*, lam*."""
    import wlsqm.hip as whip
    case = _geometry_case(name)
    c, T = case["c"], case["T"]
    sy = c["sy"]
    S, b = _t(sy["S"]).requires_grad_(), _t(sy["b"])
    op = whip.StencilOperator(sy["dim"], sy["order"], _t(sy["S"]), _t(sy["hoods"]), _t(sy["nk"]), _t(sy["knowns"]), _t(sy["wm"]), _t(sy["rows"]))
    solver = whip.StencilSystemSolver(op, sy["coupling"], diag=sy["diag"])
    calls = _count_calls(monkeypatch, whip)
    x = whip.differentiable_stencil_system_solve(solver, b, S=S, maxiter=c["cap"])
    assert calls == ["solve"]
    del calls[:]
    (x * _t(c["w"])).sum().backward()
    assert calls == ["solve-transposed"] + ["fit_cloud_device", "fit_cloud_geometry_adjoint_device"] * sy["m"] and b.grad is None
    assert tuple(S.grad.shape) == tuple(S.shape)
    dist = np.abs(S.grad.cpu().numpy() - T).max()
    print("%s dL/dS: |T|_inf %.3e, a %.3e, b_dev %.3e, distance %.3e, bound %.3e"
          % (name, np.abs(T).max(), case["a"], case["b_dev"], dist, 8 * case["a"] + 2 * case["b_dev"]))
    assert dist <= 8 * case["a"] + 2 * case["b_dev"]
    solver.close(); op.close()


def test_two_chained_steps_share_one_operator_and_solver(wlsqm):
    import torch
    import wlsqm.hip as whip
    name = "reaction-2D-n130"
    case = _geometry_case(name)
    c = case["c"]
    sy = c["sy"]
    n = sy["n"]
    SA_, SB_ = sy["S"], sy["S"] + 0.05 * n ** -0.5 * np.random.default_rng(79).standard_normal(sy["S"].shape)
    build = lambda S: whip.StencilOperator(2, 2, _t(S), _t(sy["hoods"]), _t(sy["nk"]), _t(sy["knowns"]), _t(sy["wm"]), _t(sy["rows"]))
    w = _t(c["w"])
    cp1, cp2 = sy["coupling"], 1.25 * sy["coupling"]

    def two_steps(solver1, solver2):
        S1, S2, b = _t(SA_).requires_grad_(), _t(SB_).requires_grad_(), _t(sy["b"]).requires_grad_()
        c1, c2 = torch.from_numpy(cp1.copy()).requires_grad_(), torch.from_numpy(cp2.copy()).requires_grad_()
        x1 = whip.differentiable_stencil_system_solve(solver1, b, S=S1, coupling=c1, maxiter=c["cap"])
        x2 = whip.differentiable_stencil_system_solve(solver2, x1, S=S2, coupling=c2, maxiter=c["cap"])
        (x2 * w).sum().backward()
        return x2.detach(), b.grad, S1.grad, S2.grad, c1.grad, c2.grad

    ops = [build(SB_), build(SA_), build(SB_)]                           # the shared one starts at SB: the first step's update moves it
    solvers = [whip.StencilSystemSolver(o, cp1, diag=sy["diag"]) for o in ops]
    shared = two_steps(solvers[0], solvers[0])
    apart = two_steps(solvers[1], solvers[2])
    assert torch.equal(bits(shared[0]), bits(apart[0])) and torch.equal(bits(shared[1]), bits(apart[1]))
    for got, want, what in ((shared[2], apart[2], "S1"), (shared[3], apart[3], "S2")):
        dist = float((got - want).abs().max())
        print("%s: shared against separate operators, distance %.3e, bound %.3e" % (what, dist, 2 * case["b_dev"]))
        assert dist <= 2 * case["b_dev"]
    assert float(shared[2].abs().max()) > 0 and float(shared[3].abs().max()) > 0
    # coupling's gradient is the operator's deterministic product and a contraction of the same tensors: the same values
    for got, want in ((shared[4], apart[4]), (shared[5], apart[5])):
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    for o in solvers + ops:
        o.close()


def test_failure_paths(wlsqm):
    import torch
    import wlsqm.hip as whip
    c = _case("random-m3")
    sy, op = c["sy"], c["op"]
    n, mm = sy["n"], sy["m"]
    solver = whip.StencilSystemSolver(op, sy["coupling"], diag=_t(c["D"]))
    b = _t(sy["b"]).requires_grad_()
    with pytest.raises(RuntimeError, match="the forward solve did not converge: status 1, SolveInfo\\(status=1, iterations=1"):
        whip.differentiable_stencil_system_solve(solver, b, maxiter=1)
    # a forward that converges at once from the solution, an adjoint that cannot within the same single iteration
    x0 = _zeros(n, mm)
    assert solver.solve(_t(sy["b"]), x0, rtol=1e-12, maxiter=4 * c["cap"]).status == 0
    x = whip.differentiable_stencil_system_solve(solver, b, x0=x0, maxiter=1)
    assert solver.info().iterations == 0 and torch.equal(bits(x.detach()), bits(x0))
    with pytest.raises(RuntimeError, match="the adjoint solve did not converge: status 1"):
        (x * _t(c["w"])).sum().backward()
    assert b.grad is None
    # a zero coupled diagonal: unknown (5, 1) has D_11 = 0 and no own entry; status 4 and a RuntimeError, never a fault
    st = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in sy["st"].items()}
    st["nk"][5], st["own_mask"][5] = 0, False
    op0 = _operator(whip, st)
    d = sy["diag"].copy()
    d[1, 1, 5] = 0.0
    zero_diag = whip.StencilSystemSolver(op0, sy["coupling"], diag=_t(d))
    with pytest.raises(RuntimeError, match="the forward solve did not converge: status 4"):
        whip.differentiable_stencil_system_solve(zero_diag, b)
    lam = _zeros(n, mm)
    info = zero_diag.solve(_t(c["w"]), lam, transpose=True)              # the transposed start finds the same diagonal
    assert info.status == KR.DIAGONAL and info.iterations == 0 and bool((lam == 0.0).all())
    # inside a capture: the existing refusal
    refused = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="differentiable_stencil_system_solve reads the solve's scalars on the host and the stream is capturing"):
        with torch.cuda.graph(refused, stream=torch.cuda.Stream()):
            whip.differentiable_stencil_system_solve(solver, b)
    torch.cuda.synchronize()
    x = whip.differentiable_stencil_system_solve(solver, b, maxiter=c["cap"])                  # the capture ended cleanly
    assert solver.info().status == 0
    with pytest.raises(ValueError, match="S and coefficients are two ways"):
        whip.differentiable_stencil_system_solve(solver, b, S=_t(np.zeros((n, 2))), coefficients=op.coefficients())
    with pytest.raises(RuntimeError, match="made from coefficients: there is no fit to redo"):
        whip.differentiable_stencil_system_solve(solver, b, S=_t(np.zeros((n, 2))))
    zero_diag.close(); solver.close(); op0.close()
