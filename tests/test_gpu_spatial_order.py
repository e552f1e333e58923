"""GPU tests of wlsqm.hip.SpatialOrder (csrc/order.hip: "order-keys", "order-inverse", "order-relabel").

  1. keys, perm, inverse and keys_of against the numpy statement (tests/_order_ref.py), bit for bit;
  2. restore(take(t)) is t; 3. neighbour lists renumbered, against the statement and against a fresh search on the sorted cloud;
  4. the fit of the reordered cloud is the same fit, bit for bit; 5. the reordered operator is P A P^T;
  6. the solver gains what the host rehearsal says; 7. capture; 8. statuses, not faults.
"""
import numpy as np
import pytest

import _krylov_block_ref as KB
import _krylov_ref as KR
import _order_ref as O
import _stencil_ref as R
from _device_helpers import bits, dev as _t, nan as _nan, wlsqm  # noqa: F401 (fixture)
from test_gpu_krylov import _build
from test_gpu_krylov_block import _held_to_the_reference

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 300, 65537)


def _halton(n, dim, seed=0):
    """The Halton points of bases 2, 3, 5 in [0, 1)^dim, shuffled."""
    out = np.empty((n, dim))
    for m, base in enumerate((2, 3, 5)[:dim]):
        i = np.arange(1, n + 1)
        f, r = 1.0, np.zeros(n)
        while i.any():
            f /= base
            r += f * (i % base)
            i //= base
        out[:, m] = r
    return out[np.random.default_rng([3, n, dim, seed]).permutation(n)]


def _cloud(n, dim, seed=0):
    S = _halton(n, dim, seed)
    return np.ascontiguousarray(S[:, 0]) if dim == 1 else S


def _probes(S, rng):
    """Points around and outside the box of S, with a NaN, an infinity and the corners."""
    P = O.as_points(S)
    lo, hi = O.box(P)
    X = lo + (hi - lo) * (rng.random((97, P.shape[1])) * 3.0 - 1.0)
    X[0], X[1], X[2], X[3] = lo, hi, np.inf, -np.inf
    X[4, -1] = np.nan
    return np.ascontiguousarray(X[:, 0]) if S.ndim == 1 else X


def _against_the_statement(whip, S, what):
    order = whip.SpatialOrder(_t(S))
    assert whip.last_kernel() == "order-inverse"
    n = len(S)
    key, perm, inverse = O.order(S)
    lo, hi = O.box(S)
    assert order.npoints == n and order.dimension == O.as_points(S).shape[1] and order.bits == O.BITS[order.dimension]
    assert order.lo == tuple(lo) and order.hi == tuple(hi), what
    got_perm = order.perm.cpu().numpy()
    assert np.array_equal(np.sort(got_perm), np.arange(n)), what                   # a permutation
    got_key = order.keys.cpu().numpy()
    assert (got_key[1:] >= got_key[:-1]).all(), what                               # ascending (compared: 1D keys span int64)
    ties = got_key[1:] == got_key[:-1]
    assert (got_perm[1:][ties] > got_perm[:-1][ties]).all(), what                  # ties by index
    assert np.array_equal(got_key, key), what
    assert np.array_equal(got_perm, perm) and np.array_equal(order.inverse.cpu().numpy(), inverse), what
    assert order.perm.dtype == order.inverse.dtype == order.keys.dtype and str(order.keys.dtype) == "torch.int64"
    # keys_of: the cloud's own points, and probes outside the box
    assert np.array_equal(order.keys_of(_t(S)).cpu().numpy()[perm], key), what
    assert whip.last_kernel() == "order-keys"
    X = _probes(S, np.random.default_rng([9, n]))
    got = order.keys_of(_t(X)).cpu().numpy()
    assert np.array_equal(got, O.keys(X, lo, hi)), what
    assert got[4] == O.LARGEST[order.dimension] and got[0] == got[3] and got[1] == got[2] and (np.delete(got, 4) <= got[1]).all()
    return order


@pytest.mark.parametrize("dim,p,origin,s,flat", O.lattice_cases())
def test_lattices_against_the_statement_and_the_integer_truth(wlsqm, dim, p, origin, s, flat):
    import wlsqm.hip as whip
    S, J = O.lattice(dim, p, origin, s, rng=np.random.default_rng([5, dim, p, s + 1000]), flat=flat)
    order = _against_the_statement(whip, S, "lattice %s" % ((dim, p, origin, s, flat),))
    B = O.BITS[dim]
    want = O.interleave(O.lattice_cells(J, p, B), B)
    assert np.array_equal(order.keys_of(_t(S)).cpu().numpy(), want)


@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_clouds_against_the_statement(wlsqm, n, dim):
    import wlsqm.hip as whip
    _against_the_statement(whip, _cloud(n, dim), "halton n %d dim %d" % (n, dim))


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_far_tiny_huge_coincident_and_duplicated_clouds(wlsqm, dim):
    import wlsqm.hip as whip
    S = _cloud(300, dim)
    for what, T in (("at 1e6", S + 1e6), ("2^-400", np.ldexp(S - 0.25, -400)), ("2^400", np.ldexp(S - 0.25, 400)),
                    ("coincident", np.full_like(S, 0.625)), ("duplicates", S[np.random.default_rng(dim).integers(0, 40, 300)])):
        order = _against_the_statement(whip, np.ascontiguousarray(T), "%s dim %d" % (what, dim))
        if what == "coincident":
            assert np.array_equal(order.perm.cpu().numpy(), np.arange(300))
    if dim == 1:
        tiny = 5e-324                                                      # (+-1e300 would be outside the domain of knn)
        x = np.array([0.0, -0.0, tiny, -tiny, -3 * tiny, 1.0, -1.0, -0.0, 0.0, 2.2250738585072014e-308, -1e150, 1e150, 7.5, 7.5])
        order = _against_the_statement(whip, x, "1D signed zeros and subnormals")
        assert np.array_equal(order.perm.cpu().numpy(), np.argsort(x + 0.0, kind="stable"))
    # the permutation does not change under a power of two
    base = whip.SpatialOrder(_t(S)).perm
    for e in (40, -40):
        import torch
        assert torch.equal(whip.SpatialOrder(_t(np.ldexp(S, e))).perm, base)


# ---- 2. round trip -----------------------------------------------------------------------------------------------------------------------

def test_restore_of_take_is_the_tensor(wlsqm):
    import torch
    import wlsqm.hip as whip
    n = 300
    order = whip.SpatialOrder(_t(_cloud(n, 3)))
    perm = order.perm
    g = torch.Generator(device="cuda").manual_seed(5)
    a = torch.randn((n, 3), dtype=torch.float64, device="cuda", generator=g)
    a[7, 1] = float("nan")
    cases = [(a, 0), (torch.arange(n, dtype=torch.int32, device="cuda") * 7 - 50, 0), (torch.rand(n, device="cuda", generator=g) < 0.5, 0),
             (torch.randn((5, n), dtype=torch.float64, device="cuda", generator=g), 1), (torch.randn((5, n), dtype=torch.float64, device="cuda", generator=g), -1)]
    for t, d in cases:
        moved = order.take(t, dim=d)
        assert moved.dtype == t.dtype and moved.shape == t.shape
        assert torch.equal(moved.view(torch.uint8) if t.dtype == torch.bool else moved.contiguous().view(torch.uint8),
                           t.index_select(d, perm).contiguous().view(torch.uint8))
        back = order.restore(moved, dim=d)
        assert torch.equal(back.contiguous().view(torch.uint8), t.contiguous().view(torch.uint8))
        out = torch.empty_like(moved)
        assert order.take(t, dim=d, out=out) is out and torch.equal(out.contiguous().view(torch.uint8), moved.contiguous().view(torch.uint8))
    assert torch.equal(order.take(torch.arange(n, device="cuda")), perm)


# ---- 3. lists ----------------------------------------------------------------------------------------------------------------------------

def _sorted_d2(S, hoods, nk=None):
    """Per row the ascending squared distances of the listed points (inf in the padding)."""
    d2 = ((S[hoods] - S[:, None, :]) ** 2).sum(axis=2)
    if nk is not None:
        d2 = np.where(np.arange(hoods.shape[1])[None, :] < nk[:, None], d2, np.inf)
    return np.sort(d2, axis=1)


@pytest.mark.parametrize("dim,K", [(2, 24), (3, 40)])
def test_lists_of_a_search(wlsqm, dim, K):
    import torch
    import wlsqm.hip as whip
    n = 1000
    S = _cloud(n, dim, seed=1)
    S_d = _t(S)
    order = whip.SpatialOrder(S_d)
    perm, inverse = order.perm.cpu().numpy(), order.inverse.cpu().numpy()
    hoods = whip.knn(S_d, K)
    got = order.hoods(hoods)
    assert whip.last_kernel() == "order-relabel" and got.dtype == torch.int32 and tuple(got.shape) == (n, K)
    want, bad = O.relabel(hoods.cpu().numpy(), None, inverse, row_perm=perm)
    assert bad == 0 and np.array_equal(got.cpu().numpy(), want)
    # the same neighbourhoods as a search on the sorted cloud: the multiset of distances per row (tie order at the K-th place is unspecified)
    S2_d = order.take(S_d).contiguous()
    again = whip.knn(S2_d, K).cpu().numpy()
    S2 = S2_d.cpu().numpy()
    assert np.array_equal(S2, S[perm])
    assert np.array_equal(_sorted_d2(S2, want), _sorted_d2(S2, again))
    # a ragged ball result: padding holds the row's own new number
    r = {2: 0.1, 3: 0.2}[dim]
    bh, bnk = whip.ball(S_d, r, K)
    got = order.hoods(bh, bnk)
    want, bad = O.relabel(bh.cpu().numpy(), bnk.cpu().numpy(), inverse, row_perm=perm)
    assert bad == 0 and np.array_equal(got.cpu().numpy(), want)
    nk2 = order.take(bnk)
    assert int(bnk.min()) < int(bnk.max())                                                      # ragged indeed
    bh2, bnk2 = whip.ball(S2_d, r, K)
    assert torch.equal(bnk2, nk2)
    assert np.array_equal(_sorted_d2(S2, want, nk2.cpu().numpy()), _sorted_d2(S2, bh2.cpu().numpy(), bnk2.cpu().numpy()))
    pad = np.arange(K)[None, :] >= nk2.cpu().numpy()[:, None]
    assert np.array_equal(want[pad], np.broadcast_to(np.arange(n)[:, None], (n, K))[pad])
    # relabel: a point_index, and the lists of a subset of the cases, rows unmoved
    pidx = torch.from_numpy(np.random.default_rng(2).integers(0, n, 77).astype(np.int32)).cuda()
    assert np.array_equal(order.relabel(pidx).cpu().numpy(), inverse[pidx.cpu().numpy()].astype(np.int32))
    sub = bh[100:177]
    got = order.relabel(sub, bnk[100:177])
    want, bad = O.relabel(sub.cpu().numpy(), bnk[100:177].cpu().numpy(), inverse, own=np.full(77, -1))
    assert bad == 0 and np.array_equal(got.cpu().numpy(), want)


def test_an_entry_that_names_no_point_is_a_status(wlsqm):
    import wlsqm.hip as whip
    n, K = 300, 7
    S_d = _t(_cloud(n, 2))
    order = whip.SpatialOrder(S_d)
    hoods = whip.knn(S_d, K)
    clean = order.hoods(hoods).cpu().numpy()
    hoods[17, 3] = n
    i = int(order.inverse[17])
    with pytest.raises(ValueError, match=r"a live entry names a point outside 0 \.\. npoints - 1 = %d" % (n - 1)):
        order.hoods(hoods)
    got = order.hoods(hoods, check=False).cpu().numpy()
    assert got[i, 3] == -1
    got[i, 3] = clean[i, 3]
    assert np.array_equal(got, clean)
    with pytest.raises(ValueError, match="a live entry names a point outside"):
        order.relabel(hoods[17])
    hoods[17, 3] = -5
    assert order.relabel(hoods[17], check=False).cpu().numpy()[3] == -1
    # padding is not looked at
    nk = _t(np.full(n, 3, np.int32))
    assert np.array_equal(order.hoods(hoods, nk).cpu().numpy()[:, :3], clean[:, :3])


# ---- 4. the fit is the same fit ----------------------------------------------------------------------------------------------------------

_fits = {}


def _fit_inputs(dim, K):
    if (dim, K) not in _fits:
        import wlsqm as W
        import wlsqm.hip as whip
        n = 1000
        S = _cloud(n, dim, seed=2)
        P = O.as_points(S)
        F = np.sin(3.0 * P[:, 0]) + (P[:, -1] - 0.3) ** 2 + 0.5 * P.prod(axis=1)
        S_d = _t(S)
        _fits[(dim, K)] = dict(n=n, S=S_d, F=_t(F), hoods=whip.knn(S_d, K), nk=_t(np.full(n, K, np.int32)), knowns=_t(np.zeros(n, np.int64)),
                               wm=_t(np.full(n, W.WEIGHT_CENTER, np.int32)), order=whip.SpatialOrder(S_d))
    return _fits[(dim, K)]


@pytest.mark.parametrize("dim,K,mode", [(2, 24, None), (3, 40, None), (2, 24, "accurate")])
def test_the_fit_of_the_reordered_cloud_is_the_same_fit(wlsqm, dim, K, mode):
    import torch
    import wlsqm.hip as whip
    m = _fit_inputs(dim, K)
    order, n = m["order"], m["n"]
    no = {2: 6, 3: 10}[dim]
    fi = torch.zeros((n, no), dtype=torch.float64, device="cuda")
    whip.fit_cloud_device(dim, 2, m["S"], m["F"], m["hoods"], fi, m["nk"], m["knowns"], m["wm"], strict=mode)
    given_kernel = whip.last_kernel()
    S2, hoods2, nk2, knowns2, wm2 = order.cloud(m["S"], m["hoods"], m["nk"], m["knowns"], m["wm"])
    fi2 = torch.zeros((n, no), dtype=torch.float64, device="cuda")
    whip.fit_cloud_device(dim, 2, S2, order.take(m["F"]).contiguous(), hoods2, fi2, nk2, knowns2, wm2, strict=mode)
    assert whip.last_kernel() == given_kernel
    back = order.restore(fi2)
    assert torch.isfinite(fi).all()
    differ = int((bits(back) != bits(fi)).any(dim=1).sum())
    print("dim %d K %d mode %s (%s): %d of %d cases differ in some bit" % (dim, K, mode, given_kernel, differ, n))
    assert differ == 0


# ---- 5. the operator is the same operator --------------------------------------------------------------------------------------------------

def _permuted(A, perm):
    return A[np.ix_(perm, perm)]


def test_the_reordered_operator_of_a_fit(wlsqm):
    import torch
    import wlsqm.hip as whip
    sy = KR.system("2D-tau0.25-n1000")
    op, _ = _build(whip, sy)
    n = sy["n"]
    order = whip.SpatialOrder(_t(sy["S"]))
    perm = order.perm.cpu().numpy()
    op2 = order.operator(op)
    assert op2.ncases == op2.npoints == n and op2.nop == op.nop and op2.K == op.K
    F = _t(np.random.default_rng(3).standard_normal(n))
    y, y2 = op.apply(F), op2.apply(order.take(F))
    assert torch.equal(bits(order.restore(y2, dim=1)), bits(y))
    A, A2 = op.to_sparse_csr(0).to_dense().cpu().numpy(), op2.to_sparse_csr(0).to_dense().cpu().numpy()
    assert np.array_equal(A2, _permuted(A, perm))
    # the transposed product sums a column's entries in case order, which the renumbering changes: held to the bound of a sum of that
    # many terms in any order, 2 gamma_len sum |a_ij g_i|
    g = _t(np.random.default_rng(4).standard_normal((1, n)))
    z, z2 = op.apply_transpose(g).cpu().numpy(), order.restore(op2.apply_transpose(order.take(g, dim=1)), dim=-1).cpu().numpy()
    count = (A != 0).sum(axis=0)
    bound = 2 * R.gamma(count + 1) * (np.abs(A).T @ np.abs(g.cpu().numpy()[0]))
    assert (np.abs(z - z2).ravel() <= bound).all() and np.abs(z).max() > 0
    op2.close()


@pytest.mark.parametrize("n", [1, 65, 300])
def test_the_reordered_operator_of_a_random_structure(wlsqm, n):
    """Ragged rows, empty rows, own entries on half of the rows, duplicated and self columns, -1 / npoints in the padding."""
    import torch
    import wlsqm.hip as whip
    st = KR.square_structure(n, 9, seed=31)
    op = whip.StencilOperator.from_coefficients(_t(st["hoods"]), _t(st["nk"]), _t(st["slots"]), n, own=_t(st["own"]), own_mask=_t(st["own_mask"]))
    order = whip.SpatialOrder(_t(_cloud(n, 3, seed=4)))
    perm = order.perm.cpu().numpy()
    op2 = order.operator(op)
    F = _t(np.random.default_rng(5).standard_normal((3, n)))
    assert torch.equal(bits(order.restore(op2.apply(order.take(F, dim=1)), dim=-1)), bits(op.apply(F)))
    rows = R.rows_of(st["hoods"], st["nk"], st["slots"], st["own"], st["own_mask"], st["pts"])
    A, tol = R.dense_bound(rows, n, 0)                                     # duplicates are summed by to_sparse_csr in its own order
    A2 = op2.to_sparse_csr(0).to_dense().cpu().numpy()
    assert (np.abs(A2 - _permuted(A, perm)) <= _permuted(tol, perm)).all()
    s1, o1 = op.coefficients()
    s2, o2 = op2.coefficients()
    assert torch.equal(bits(s2), bits(s1[:, order.perm])) and torch.equal(bits(o2), bits(o1[:, order.perm]))


def test_the_reordered_operator_keeps_its_known_derivatives(wlsqm):
    """An operator of a fit with known DOFs other than F: the reordered one takes known= in the new order and gives the same bits."""
    import torch
    import wlsqm.hip as whip
    from test_gpu_stencil import _small_cloud
    n = 70
    geo = tuple(_t(a) for a in _small_cloud(n))
    op = whip.StencilOperator(2, 2, *geo, whip.stencil_rows(2, 2, "gradient", "laplacian", device="cuda"))
    assert op.has_known_derivatives and op.nop == 3
    order = whip.SpatialOrder(geo[0])
    op2 = order.operator(op)
    assert op2.has_known_derivatives and (op2.dimension, op2.order, op2.no) == (2, 2, 6)
    assert torch.equal(bits(op2.known_coef), bits(op.known_coef[:, order.perm]))
    rng = np.random.default_rng(33)
    for lead in ((), (2,)):
        F, known = _t(rng.standard_normal(lead + (n,))), _t(rng.standard_normal(lead + (n, 6)))
        with pytest.raises(ValueError, match="pass known="):
            op2.apply(order.take(F, dim=-1))
        want = op.apply(F, known=known)
        got = op2.apply(order.take(F, dim=-1).contiguous(), known=order.take(known, dim=-2).contiguous())
        assert want.shape == lead + (3, n) and torch.equal(bits(order.restore(got, dim=-1)), bits(want))
    # autograd: dL/dknown per case is the same sum; dL/dF is the transposed product, equal within the bound of a sum in another order
    F, known, g = _t(rng.standard_normal(n)), _t(rng.standard_normal((n, 6))), _t(rng.standard_normal((3, n)))
    F1, k1 = F.clone().requires_grad_(), known.clone().requires_grad_()
    whip.differentiable_stencil_apply(op, F1, k1).backward(g)
    F2, k2 = order.take(F).contiguous().requires_grad_(), order.take(known).contiguous().requires_grad_()
    whip.differentiable_stencil_apply(op2, F2, k2).backward(order.take(g, dim=1).contiguous())
    assert torch.equal(bits(order.restore(k2.grad)), bits(k1.grad)) and float(k1.grad.abs().max()) > 0
    A = np.stack([op.to_sparse_csr(o).to_dense().cpu().numpy() for o in range(3)])
    bound = 2 * R.gamma((A != 0).sum(axis=(0, 1)) + 1) * np.einsum("oji,oj->i", np.abs(A), np.abs(g.cpu().numpy()))
    assert (np.abs(order.restore(F2.grad).cpu().numpy() - F1.grad.cpu().numpy()) <= bound).all()
    op2.close(); op.close()


def test_operators_that_are_refused(wlsqm):
    import wlsqm.hip as whip
    n = 130
    st = R.random_structure(n - 30, n, 9, 1, seed=3)                       # not square, with a point_index
    op = whip.StencilOperator.from_coefficients(_t(st["hoods"]), _t(st["nk"]), _t(st["slots"]), n, own=_t(st["own"]), own_mask=_t(st["own_mask"]),
                                                point_index=_t(st["pts"]))
    order = whip.SpatialOrder(_t(_cloud(n, 2)))
    with pytest.raises(ValueError, match="square operator whose row j names point j"):
        order.operator(op)
    sq = KR.square_structure(n, 9, seed=31)
    op = whip.StencilOperator.from_coefficients(_t(sq["hoods"]), _t(sq["nk"]), _t(sq["slots"]), n, own=_t(sq["own"]), own_mask=_t(sq["own_mask"]),
                                                point_index=_t(sq["pts"]))
    with pytest.raises(ValueError, match="with a point_index"):
        order.operator(op)
    with pytest.raises(ValueError, match="op must be a StencilOperator"):
        order.operator(None)


# ---- 6. the solver gains what the rehearsal says ---------------------------------------------------------------------------------------------

def _solve_both(whip, name):
    """Block-16 solves of the system `name` as given (random order) and through order.operator: (counts, restored solutions agree)."""
    import torch
    sy = KR.system(name)
    n = sy["n"]
    op, args = _build(whip, sy)
    order = whip.SpatialOrder(_t(sy["S"]))
    perm = order.perm.cpu().numpy()
    op2 = order.operator(op)
    M = KR.dense_of(sy, op.to_sparse_csr(0).to_dense().cpu().numpy())
    M2 = KR.dense_of(sy, op2.to_sparse_csr(0).to_dense().cpu().numpy())
    assert np.array_equal(M2, M[np.ix_(perm, perm)])
    b = _t(sy["b"])
    out = []
    for what, o, A, rhs in (("as given", op, M, b), ("reordered", op2, M2, order.take(b))):
        # the cap: twice the reference recurrence's count on this very matrix, as tests/_krylov_block_ref.CAPS are made
        _, its_r, st_r, _ = KB.solve_ref(A, rhs.cpu().numpy(), 16)
        assert st_r == KR.CONVERGED
        x = torch.zeros(n, dtype=torch.float64, device="cuda")
        solver = whip.StencilSolver(o, preconditioner=whip.BlockJacobi(16), **args)
        info = solver.solve(rhs, x, rtol=KR.RTOL, maxiter=2 * its_r)
        _held_to_the_reference(A, rhs.cpu().numpy(), x.cpu().numpy(), info, KB.block_preconditioner(A, 16), 2 * its_r, "%s %s" % (name, what))
        out.append((info.iterations, its_r, x))
        solver.close()
    x, x2 = out[0][2].cpu().numpy(), order.restore(out[1][2]).cpu().numpy()
    gap, room = np.linalg.norm(x - x2), np.linalg.cond(M) * KR.RTOL * np.linalg.norm(x)
    print("%-22s as given %3d (reference %3d)   reordered %3d (reference %3d)   |x - x'| %.3e, kappa rtol |x| %.3e"
          % (name, out[0][0], out[0][1], out[1][0], out[1][1], gap, room))
    return out[0][0], out[1][0], gap, room


@pytest.mark.parametrize("name", ["2D-tau1-n130", "3D-tau0.25-n1000"])
def test_the_solver_gains_from_the_order(wlsqm, name):
    import wlsqm.hip as whip
    given, reordered, gap, room = _solve_both(whip, name)
    assert reordered <= 0.75 * given, (name, given, reordered)
    assert gap <= room


@pytest.mark.parametrize("name", ["2D-dirichlet-n1000", "2D-dirichlet-n130", "3D-dirichlet-n1000", "2D-tau0.25-n1000"])
def test_the_other_systems_converge_either_way(wlsqm, name):
    """Printed, not held to a ratio (the host rehearsal has 63 / 43, 23 / 15, 19 / 16 and 13 / 9)."""
    import wlsqm.hip as whip
    _solve_both(whip, name)


# ---- 7. capture ------------------------------------------------------------------------------------------------------------------------------

def test_capture_and_replay(wlsqm):
    import torch
    import wlsqm.hip as whip
    n, K = 300, 12
    S = _cloud(n, 2, seed=6)
    S_d = _t(S)
    order = whip.SpatialOrder(S_d)
    hoods = whip.knn(S_d, K)
    X = _t(_probes(S, np.random.default_rng(8)))
    out_h = torch.full((n, K), -7, dtype=torch.int32, device="cuda")
    out_k = torch.full((X.shape[0],), -7, dtype=torch.int64, device="cuda")
    sub, sub_nk = hoods[40:90], _t(np.random.default_rng(9).integers(0, K + 1, 50).astype(np.int32))
    out_r = torch.full((50, K), -7, dtype=torch.int32, device="cuda")
    order.hoods(hoods, check=False, out=out_h)                                # warm-up outside the capture
    order.keys_of(X, out=out_k)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        order.hoods(hoods, check=False, out=out_h)
        order.keys_of(X, out=out_k)
        order.relabel(sub, sub_nk, check=False, out=out_r)                    # its first use: the padding was made by the constructor
    # the inputs change in place; the replay gives the eager result of the new inputs
    hoods.copy_(whip.knn(S_d, K).flip(1))
    hoods[5, 2] = n
    X.copy_(X.flip(0))
    out_h.fill_(-7); out_k.fill_(-7); out_r.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_h, order.hoods(hoods, check=False)) and int(out_h[int(order.inverse[5]), 2]) == -1
    assert torch.equal(out_k, order.keys_of(X))
    want, _ = O.relabel(sub.cpu().numpy(), sub_nk.cpu().numpy(), order.inverse.cpu().numpy(), own=np.full(50, -1))
    assert np.array_equal(out_r.cpu().numpy(), want) and torch.equal(out_r, order.relabel(sub, sub_nk, check=False))
    assert np.array_equal(out_k.cpu().numpy(), O.keys(X.cpu().numpy(), *O.box(S)))


# ---- 8. statuses, not faults -----------------------------------------------------------------------------------------------------------------

def test_refusals_that_need_a_device(wlsqm):
    import torch
    import wlsqm.hip as whip
    n = 130
    S = _cloud(n, 2)
    for bad in (np.nan, np.inf, -np.inf):
        T = S.copy()
        T[77, 1] = bad
        with pytest.raises(ValueError, match="non-finite coordinates"):
            whip.SpatialOrder(_t(T))
    with pytest.raises(ValueError, match="squared distances overflow double precision"):
        whip.SpatialOrder(_t(np.ldexp(S, 520)))
    with pytest.raises(ValueError, match="S must be contiguous"):
        whip.SpatialOrder(_t(np.zeros((n, 4)))[:, :2])
    with pytest.raises(ValueError, match=r"S must be \(npoints,\) or \(npoints, dim\) with dim 1\.\.3"):
        whip.SpatialOrder(_t(np.zeros((n, 4))))
    with pytest.raises(ValueError, match="Buffer dtype mismatch, expected 'float64'"):
        whip.SpatialOrder(_t(S.astype(np.float32)))
    S_d = _t(S)
    order = whip.SpatialOrder(S_d)
    for f in (order.take, order.restore):
        with pytest.raises(ValueError, match="must have npoints = %d entries along dim 0" % n):
            f(torch.zeros(n + 1, device="cuda"))
        with pytest.raises(ValueError, match="must have npoints = %d entries along dim 1" % n):
            f(torch.zeros((n, 3), device="cuda"), dim=1)
    hoods = whip.knn(S_d, 5)
    with pytest.raises(ValueError, match="hoods must have npoints = %d rows" % n):
        order.hoods(hoods[:-1])
    with pytest.raises(ValueError, match="Buffer dtype mismatch, expected 'int32'"):
        order.hoods(hoods.long())
    with pytest.raises(ValueError, match="Buffer dtype mismatch, expected 'int32'"):
        order.relabel(hoods.long())
    with pytest.raises(ValueError, match="hoods must have a contiguous last axis"):
        order.hoods(whip.knn(S_d, 6)[:, ::2])
    with pytest.raises(ValueError, match="nk has 5 rows, fewer than the %d cases of the batch" % n):
        order.hoods(hoods, _t(np.full(5, 5, np.int32)))
    with pytest.raises(ValueError, match=r"out must be a contiguous int32 device tensor of shape \(%d, 5\)" % n):
        order.hoods(hoods, out=torch.zeros((n, 6), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="X must have 2 coordinates per point"):
        order.keys_of(_t(np.zeros((4, 3))))
    sq = KR.square_structure(n + 1, 9, seed=31)
    op = whip.StencilOperator.from_coefficients(_t(sq["hoods"]), _t(sq["nk"]), _t(sq["slots"]), n + 1, own=_t(sq["own"]), own_mask=_t(sq["own_mask"]))
    with pytest.raises(ValueError, match="of npoints = %d; got ncases = %d" % (n, n + 1)):
        order.operator(op)
