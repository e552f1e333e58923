"""GPU tests of the stencil operators (wlsqm.hip.StencilOperator, csrc/stencil.hip).

  1. the coefficients are the bits of fit_cloud_adjoint_device, the padding exact zeros;
  2. the kernel on random structures against the exact row sum, within gamma_n sum |val x| (tests/_stencil_ref.py), n = len + 1
     (len + 2 with alpha and beta: one more term), with everything that must never be read poisoned with NaN;
  3. end to end against the mpmath truth of the fit under criteria (a) and (b) of DESIGN section 12, the reference being the
     sensitivities of fit_cloud_device contracted with F in fp64 numpy, in the per-case scale s_j = sum |c_k F_k|;
  4. the transposed product; 5. the CSR export; 6. autograd; 7. graph capture.
Figures measured on an MI355X are in DESIGN.md section 16.
"""
import numpy as np
import pytest

import _adversarial as A
import _parity as P
import _stencil_ref as R
from _device_helpers import bits, dev as _t, nan as _nan, same_bits as _same_bits, wlsqm  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

N = A.N_OP
WORKERS = 12
SHAPES = ((1, 2, 8), (2, 2, 32), (2, 4, 64), (3, 2, 40))
EDGES = ("tiny_edge", "huge_edge")              # reported, not asserted (DESIGN section 15 narrows the range the same way)
_ids = lambda s: "%dD-o%d-K%d" % s


def _cloud(f, dim, order, K):
    b = A.op_batch(f, dim, order, K)
    S, F, hoods, pidx = (b["S"], b["F"], b["hoods"], b["pidx"]) if f == "lattice" else A.point_table(b)
    return b, S, F, hoods, pidx


# ---- 1. coefficients ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_coefficients_are_the_bits_of_the_adjoint(wlsqm, shape):
    import torch
    import wlsqm.hip as whip
    dim, order, K = shape
    for f in ("plain", "lattice"):
        b, S, F, hoods, pidx = _cloud(f, dim, order, K)
        no, npoints = b["no"], len(F)
        rng = np.random.default_rng([dim, order, K, len(f)])
        nk = rng.integers(no, K + 1, N).astype(np.int32)
        nk[0], nk[1], nk[2] = 0, K, K
        hoods = hoods.copy()
        pad = np.arange(K)[None, :] >= nk[:, None]
        hoods[pad] = np.where((np.arange(N)[:, None] + np.arange(K)[None, :]) % 2 == 0, -1, npoints)[pad]
        kn = b["kn"].copy()
        kn[5::7] = 3                                                    # b_F | b_X: a known derivative
        geo = (_t(S), _t(hoods), _t(nk), _t(kn), _t(b["wm"]))
        for rows in (rng.uniform(-1, 1, (2, N, no)), rng.uniform(-1, 1, (3, no))):
            op = whip.StencilOperator(dim, order, *geo, _t(rows), point_index=_t(pidx))
            slots, own = (x.cpu().numpy() for x in op.coefficients())
            nop = rows.shape[0]
            assert slots.shape == (nop, N, K) and own.shape == (nop, N) and (op.nop, op.ncases, op.npoints) == (nop, N, npoints)
            assert np.all(slots[:, pad] == 0.0), "padding of the coefficients"
            fknown = (kn & 1) == 1
            assert np.all(own[:, ~fknown] == 0.0)
            for o in range(nop):
                g = _t(rows[o] if rows.ndim == 3 else np.broadcast_to(rows[o], (N, no)))
                want, gfi = _nan(N, K), _nan(N, no)
                whip.fit_cloud_adjoint_device(dim, order, *geo, g, point_index=_t(pidx), grad_fi=gfi, slots=want)
                want, gfi = want.cpu().numpy(), gfi.cpu().numpy()
                assert _same_bits(slots[o][~pad], want[~pad]), (f, shape, o)
                assert _same_bits(own[o][fknown], gfi[fknown, 0]), (f, shape, o)
                kc = gfi.copy()
                kc[fknown, 0] = 0.0
                assert _same_bits(op.known_coef[o].cpu().numpy(), kc), (f, shape, o)
            assert op.has_known_derivatives
            live = int(nk.sum() + fknown.sum())
            assert op.fill == live / op._m["total"] and op.fill_transposed is None and op.memory_used() > 0
            with pytest.raises(ValueError, match="pass known="):
                op.apply(_t(F))
            op.close()
    torch.cuda.synchronize()


# ---- 2. the kernel against the exact sum ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nrows", (1, 63, 64, 65, 130))
def test_kernel_against_the_exact_sum(wlsqm, nrows):
    import torch
    import wlsqm.hip as whip
    K, npoints, NOP, NR = 66, 200, 5, 5
    st = R.random_structure(nrows, npoints, K, NOP, seed=11)
    rows = R.rows_of(st["hoods"], st["nk"], st["slots"], st["own"], st["own_mask"], st["pts"])
    lens = np.array([len(r) for r in rows])
    assert lens.min() == 0 or nrows == 1
    assert lens.max() >= 66
    rng = np.random.default_rng([7, nrows])
    X = rng.standard_normal((NR, npoints)) * 10.0 ** rng.integers(-2, 3, (NR, npoints))
    X[:, ~R.named(rows, npoints)] = np.nan                              # whatever no live entry names is never read
    assert np.isnan(X).any()
    exact, mag = R.exact_apply(rows, X, NOP)
    bound = R.gamma(lens + 1) * mag
    alpha, beta = -0.75, 1.5
    Y0 = rng.standard_normal((NR, NOP, nrows))
    exact2, mag2 = R.exact_apply(rows, X, NOP, alpha, beta, Y0)
    bound2 = R.gamma(lens + 2) * mag2
    seen = {}
    for nop in (1, 3, 5):
        op = whip.StencilOperator.from_coefficients(_t(st["hoods"]), _t(st["nk"]), _t(st["slots"][:nop]), npoints, own=_t(st["own"][:nop]),
                                                    own_mask=_t(st["own_mask"]), point_index=_t(st["pts"]))
        m = R.pack(rows, NOP)
        assert np.array_equal(op._m["col"].cpu().numpy(), m["col"]) and _same_bits(op._val.cpu().numpy(), m["val"][:nop])
        for nr in (1, 2, 5):
            Xd = _t(np.ascontiguousarray(X[:nr].T)).t()                 # a transposed view of (npoints, R)
            assert Xd.shape == (nr, npoints) and (nr == 1 or Xd.stride() == (1, nr))
            out = _nan(nr, nop, nrows)                                  # beta == 0 must not read it
            op.apply(Xd, out=out)
            assert whip.last_kernel() == "stencil-apply"
            got = out.cpu().numpy()
            assert np.isfinite(got).all(), (nrows, nop, nr)
            assert np.all(np.abs(got - exact[:nr, :nop]) <= bound[:nr, :nop]), (nrows, nop, nr, np.abs(got - exact[:nr, :nop]).max())
            assert np.all(got[:, :, lens == 0] == 0.0)
            again = op.apply(Xd)
            assert torch.equal(bits(again), bits(out))
            for r in range(nr):
                for o in range(nop):                                    # the bits do not depend on the blocks an entry is summed in
                    assert _same_bits(seen.setdefault((r, o), got[r, o]), got[r, o]), (nrows, nop, nr, r, o)
            if nr == 1:
                one = op.apply(Xd[0])
                assert one.shape == (nop, nrows) and torch.equal(bits(one), bits(out[0]))
            y = _t(Y0[:nr, :nop])
            op.apply(Xd, out=y, alpha=alpha, beta=beta)
            got2 = y.cpu().numpy()
            assert np.all(np.abs(got2 - exact2[:nr, :nop]) <= bound2[:nr, :nop]), (nrows, nop, nr)
            wide = _nan(nr, nrows + 3, nop + 2)                         # out with strides of its own
            view = wide[:, :nrows, :nop].transpose(1, 2)
            op.apply(Xd, out=view)
            assert torch.equal(bits(view), bits(out)) and bool(torch.isnan(wide[:, nrows:]).all()) and bool(torch.isnan(wide[:, :, nop:]).all())
        op.close()


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------------------

_TRUTHS = {}


def _truths(shape):
    """truth_fit_mp of every family of one shape: {family: (fi (N, no), kappa (N,))}.  Computed once per module in worker processes."""
    if shape not in _TRUTHS:
        dim, order, K = shape
        step = 32
        per = N // step
        res = A.truths([(f, dim, order, K, N, lo, lo + step) for f in A.OP_FAMILIES for lo in range(0, N, step)], WORKERS)
        _TRUTHS[shape] = {f: (np.concatenate([r[0] for r in res[i * per:(i + 1) * per]]), np.concatenate([r[1] for r in res[i * per:(i + 1) * per]]))
                          for i, f in enumerate(A.OP_FAMILIES)}
    return _TRUTHS[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_end_to_end_against_the_mpmath_truth(wlsqm, shape):
    """rows = the identity: apply(F)[a, j] is DOF a of the fit of case j.  Per case and DOF the scale is s = sum_k |c_k F_k| (the own
    entry included), the error of a case the largest over its DOFs of |x - y| / s."""
    import torch
    import wlsqm.hip as whip
    dim, order, K = shape
    truths = _truths(shape)
    eps = np.finfo(np.float64).eps
    for f in A.OP_FAMILIES:
        b, S, F, hoods, pidx = _cloud(f, dim, order, K)
        no, nk, kn = b["no"], b["nk"], b["kn"]
        geo = (_t(S), _t(hoods), _t(nk), _t(kn), _t(b["wm"]))
        op = whip.StencilOperator(dim, order, *geo, torch.eye(no, dtype=torch.float64, device="cuda"), point_index=_t(pidx))
        assert not op.has_known_derivatives, f
        got = op.apply(_t(F))
        assert whip.last_kernel() == "stencil-apply"
        got = got.cpu().numpy().T
        # the route that exists today: the sensitivities of the index-based fit, contracted with F in fp64 numpy
        fi, sens = _t(b["fi0"]), torch.full((N, K, no), 777.0, dtype=torch.float64, device="cuda")
        whip.fit_cloud_device(dim, order, _t(S), _t(F), _t(hoods), fi, _t(nk), _t(kn), _t(b["wm"]), point_index=_t(pidx), sens=sens)
        sens = sens.cpu().numpy()
        live = np.arange(K)[None, :] < nk[:, None]
        fknown = (kn & 1) == 1
        sl = np.where(live[:, :, None], sens, 0.0)
        sl[fknown, :, 0] = 0.0
        Fk, Fo = np.where(live, F[np.where(live, hoods, 0)], 0.0), F[pidx]
        ref = np.einsum("jka,jk->ja", sl, np.where(fknown[:, None], Fk - Fo[:, None], Fk))     # an F-known fit subtracts the own value first
        ref[fknown, 0] = Fo[fknown]
        s = np.einsum("jka,jk->ja", np.abs(sl), np.abs(Fk)) + np.where(fknown[:, None], np.abs(sl.sum(axis=1)) * np.abs(Fo)[:, None], 0.0)
        s[fknown, 0] = np.abs(Fo[fknown])
        s[s == 0] = 1.0
        T, kappa = truths[f]

        def err(x, y):
            with np.errstate(invalid="ignore", over="ignore"):
                e = (np.abs(x - y) / s).max(axis=1)
            return np.where(np.isfinite(e), e, np.inf)

        e_cr, e_ct, e_rt = err(got, ref), err(got, T), err(ref, T)
        qc, qr = e_ct / (eps * kappa ** 2), e_rt / (eps * kappa ** 2)
        what = "stencil apply, %s %dD order %d K %d" % (f, dim, order, K)
        print("%-60s err: gpu-truth %.3g ref-truth %.3g gpu-ref %.3g   max q: gpu %.3g ref %.3g" % (what, e_ct.max(), e_rt.max(), e_cr.max(),
                                                                                                 qc.max(), qr.max()))
        if f not in EDGES:
            P.assert_scaled(e_cr, e_ct, e_rt, what)
            P.assert_q(qc, qr, kappa, what)
        op.close()


# ---- 4. the transpose, 5. CSR ------------------------------------------------------------------------------------------------------------

def _random_operator(whip, nrows=130, npoints=100, K=9, nop=3, seed=21):
    st = R.random_structure(nrows, npoints, K, nop, seed=seed, empty_slice=False)
    rows = R.rows_of(st["hoods"], st["nk"], st["slots"], st["own"], st["own_mask"], st["pts"])
    op = whip.StencilOperator.from_coefficients(_t(st["hoods"]), _t(st["nk"]), _t(st["slots"]), npoints, own=_t(st["own"]),
                                                own_mask=_t(st["own_mask"]), point_index=_t(st["pts"]))
    return st, rows, op


def test_transpose(wlsqm):
    import torch
    import wlsqm.hip as whip
    nrows, npoints, nop = 130, 100, 3
    st, rows, op = _random_operator(whip, nrows, npoints, nop=nop)
    trows = R.transpose_rows(rows, npoints)
    tlens = np.array([len(r) for r in trows])
    assert tlens.max() > 64 and tlens.min() == 0                        # one point named by more than 64 rows, some by none
    rng = np.random.default_rng(22)
    g = rng.standard_normal((2, nop, nrows))
    assert op.fill_transposed is None
    got = op.apply_transpose(_t(g))
    assert whip.last_kernel() == "stencil-apply" and got.shape == (2, npoints)
    assert 0.0 < op.fill_transposed <= 1.0 and op.prepare_transpose() is False
    tm = R.pack(trows, nop)
    assert np.array_equal(op._t["col"].cpu().numpy(), tm["col"]) and _same_bits(op._tval.cpu().numpy(), tm["val"])
    # exact: operator by operator, each in entry order; per operator len fused sums, alpha and the sum into out: nop (len + 2) roundings
    flat = R.flatten_transposed(trows, nop, nrows)
    exact, mag = R.exact_apply(flat, g.reshape(2, nop * nrows), 1)
    bound = R.gamma(nop * (tlens + 2)) * mag[:, 0]
    gn = got.cpu().numpy()
    assert np.all(np.abs(gn - exact[:, 0]) <= bound), np.abs(gn - exact[:, 0]).max()
    assert np.all(gn[:, tlens == 0] == 0.0)
    # the dense transpose, whose duplicates are summed first
    ref = np.zeros((2, npoints), np.longdouble)
    room = np.zeros((2, npoints))
    for o in range(nop):
        D = op.to_sparse_csr(o).to_dense().cpu().numpy()
        _, tol = R.dense_bound(rows, npoints, o)
        ref += np.einsum("ip,ri->rp", D.astype(np.longdouble), g[:, o].astype(np.longdouble))
        room += np.einsum("ip,ri->rp", tol, np.abs(g[:, o]))
    assert np.all(np.abs(gn - ref.astype(np.float64)) <= bound + room + 4 * np.finfo(np.float64).eps * mag[:, 0])
    # the same bits on repetition, one field alone, alpha and beta
    assert torch.equal(bits(op.apply_transpose(_t(g))), bits(got))
    assert torch.equal(bits(op.apply_transpose(_t(g[1]))), bits(got[1]))
    y0 = rng.standard_normal((2, npoints))
    y = _t(y0)
    op.apply_transpose(_t(g), out=y, alpha=0.5, beta=-2.0)
    ex2, mag2 = R.exact_apply(flat, g.reshape(2, nop * nrows), 1, 0.5, -2.0, y0[:, None, :])
    assert np.all(np.abs(y.cpu().numpy() - ex2[:, 0]) <= R.gamma(nop * (tlens + 2) + 1) * mag2[:, 0])
    # <A x, y> = <x, A^T y> within the sum of both bounds
    x, yv = rng.standard_normal(npoints), rng.standard_normal((nop, nrows))
    Ax, ATy = op.apply(_t(x)).cpu().numpy(), op.apply_transpose(_t(yv)).cpu().numpy()
    _, mag_f = R.exact_apply(rows, x[None], nop)
    _, mag_t = R.exact_apply(flat, yv.reshape(1, -1), 1)
    lens = np.array([len(r) for r in rows])
    room = float((np.abs(yv) * R.gamma(lens + 1) * mag_f[0]).sum() + (np.abs(x) * R.gamma(nop * (tlens + 2)) * mag_t[0, 0]).sum())
    assert abs(float(R.exact_dot(Ax, yv) - R.exact_dot(x, ATy))) <= room
    op.close()


def test_csr(wlsqm):
    import wlsqm.hip as whip
    nrows, npoints, nop = 130, 100, 3
    st, rows, op = _random_operator(whip, nrows, npoints, nop=nop)
    for o in (0, 2):
        csr = op.to_sparse_csr(o)
        assert tuple(csr.shape) == (nrows, npoints) and csr.layout.__str__() == "torch.sparse_csr"
        crow, col = csr.crow_indices().cpu().numpy(), csr.col_indices().cpu().numpy()
        distinct = np.array([len({c for c, _ in r}) for r in rows])
        assert crow[0] == 0 and crow[-1] == len(col) and np.array_equal(np.diff(crow), distinct)
        for i in range(nrows):
            c = col[crow[i]:crow[i + 1]]
            assert np.all(np.diff(c) > 0) and set(c.tolist()) == {c_ for c_, _ in rows[i]}
        want, tol = R.dense_bound(rows, npoints, o)
        assert (tol > 0).any()
        assert np.all(np.abs(csr.to_dense().cpu().numpy() - want) <= tol)
    with pytest.raises(ValueError):
        op.to_sparse_csr(nop)
    op.close()


# ---- 6. autograd, 7. capture -----------------------------------------------------------------------------------------------------------

def _small_cloud(n=70, K=12, seed=31, masks=(0, 1, 3)):
    rng = np.random.default_rng(seed)
    S = rng.uniform(0, 1, (n, 2))
    d2 = ((S[:, None, :] - S[None, :, :]) ** 2).sum(axis=-1)
    np.fill_diagonal(d2, np.inf)
    hoods = np.argsort(d2, axis=1, kind="stable")[:, :K].astype(np.int32)
    kn = np.array([masks[j % len(masks)] for j in range(n)], np.int64)
    return S, hoods, np.full(n, K, np.int32), kn, np.full(n, 2, np.int32)


def test_autograd(wlsqm):
    import torch
    import wlsqm.hip as whip
    n = 70
    geo = tuple(_t(a) for a in _small_cloud(n))
    op = whip.StencilOperator(2, 2, *geo, whip.stencil_rows(2, 2, "gradient", "laplacian", device="cuda"))
    assert op.has_known_derivatives and op.nop == 3
    rng = np.random.default_rng(32)
    for lead in ((), (2,)):
        F = _t(rng.standard_normal(lead + (n,))).requires_grad_()
        known = _t(rng.standard_normal(lead + (n, 6))).requires_grad_()
        out = whip.differentiable_stencil_apply(op, F, known)
        assert out.shape == lead + (3, n) and torch.equal(bits(out.detach()), bits(op.apply(F.detach(), known=known.detach())))
        assert torch.autograd.gradcheck(lambda F_, k_: whip.differentiable_stencil_apply(op, F_, k_), (F, known))
    # the gradient of F alone is the transposed product
    F = _t(rng.standard_normal(n)).requires_grad_()
    known, g = _t(rng.standard_normal((n, 6))), _t(rng.standard_normal((3, n)))
    whip.differentiable_stencil_apply(op, F, known).backward(g)
    assert torch.equal(bits(F.grad), bits(op.apply_transpose(g)))
    op.close()


def test_capture(wlsqm):
    """One explicit advection step u <- u - dt (a . grad) v as one apply with out=u, beta=1, captured on a side stream: the replay's bits
    are the eager bits; building the transposed matrix inside a capture is refused."""
    import torch
    import wlsqm.hip as whip
    n, dt = 200, 1e-3
    geo = tuple(_t(a) for a in _small_cloud(n, masks=(1,)))
    op = whip.StencilOperator(2, 2, *geo, _t(np.array([[0.0, 1.0, 0.5, 0.0, 0.0, 0.0]])))
    assert not op.has_known_derivatives
    rng = np.random.default_rng(33)
    u0, v = _t(rng.standard_normal(n)), _t(rng.standard_normal(n))
    u = u0.clone()

    def step():
        op.apply(v, out=u.view(1, n), alpha=-dt, beta=1.0)

    step()                                                               # warm-up outside the capture
    torch.cuda.synchronize()
    eager = u.clone()
    assert not torch.equal(bits(eager), bits(u0))
    u.copy_(u0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        step()
    torch.cuda.synchronize()
    assert torch.equal(bits(u), bits(u0))                                # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(u), bits(eager))
    with pytest.raises(ValueError, match="overlaps"):
        op.apply(u, out=u.view(1, n), alpha=-dt, beta=1.0)
    refused = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="call prepare_transpose before the capture"):
        with torch.cuda.graph(refused, stream=torch.cuda.Stream()):
            op.prepare_transpose()
    torch.cuda.synchronize()
    assert op.fill_transposed is None and op.prepare_transpose() is True
    op.close()
