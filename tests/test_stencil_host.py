"""Stencil operators without a GPU: the numpy statement of the SELL-64 packing and of its transpose (tests/_stencil_ref.py) against the
torch operations that pack on the device (run here on host tensors), the exact row sum and its gamma bound, stencil_rows against the
constants of wlsqm.fitter.defs, the argument checks of every new entry point on the OnDevice stub (each fails before the library is
reached), and the algebra pinned in mpmath: the coefficients that the adjoint of the fit gives for a row lambda, applied to the point
values with the own and known terms, are lambda . fi_out of the fit."""
import numpy as np
import pytest

import _adversarial as A
import _parity as P
import _stencil_ref as R
from _device_helpers import OnDevice

torch = pytest.importorskip("torch")


def _shell(st, nop):
    """A StencilOperator packed from a random structure by the library's own torch operations, on host tensors."""
    import wlsqm.hip as h
    op = h.StencilOperator.__new__(h.StencilOperator)
    op._m = op._t = op._tval = None
    t = torch.from_numpy
    op._pack(t(st["hoods"]), t(st["nk"]), t(st["slots"][:nop]), t(st["own"][:nop]), t(st["own_mask"]), t(st["pts"]).long(), st["npoints"])
    op.known_coef, op.has_known_derivatives, op.no = None, False, 0
    return op


@pytest.mark.parametrize("nrows", (1, 63, 64, 65, 130))
def test_packing_and_transpose_are_the_numpy_statement(nrows):
    nop, K, npoints = 3, 9, 150
    st = R.random_structure(nrows, npoints, K, nop, seed=1)
    rows = R.rows_of(st["hoods"], st["nk"], st["slots"], st["own"], st["own_mask"], st["pts"])
    m = R.pack(rows, nop)
    # the layout itself
    assert np.array_equal(np.diff(m["soff"]), 64 * m["width"].astype(np.int64))
    for s in range(len(m["width"])):
        assert m["width"][s] == max(len(r) for r in rows[64 * s:64 * s + 64])
    i = nrows - 1
    for e, (c, v) in enumerate(rows[i]):
        at = m["soff"][i // 64] + 64 * e + i % 64
        assert m["col"][at] == c and np.array_equal(m["val"][:, at], v)
    if nrows >= 128:
        assert m["width"][1] == 0
    # the library's packing gives the same arrays
    op = _shell(st, nop)
    for k in ("len", "width", "soff", "col"):
        assert np.array_equal(op._m[k].numpy(), m[k]), k
    assert np.array_equal(op._val.numpy(), m["val"]) and op._m["total"] == len(m["col"])
    assert op.fill == sum(len(r) for r in rows) / max(len(m["col"]), 1) or len(m["col"]) == 0
    slots, own = (x.numpy() for x in op.coefficients())
    pad = np.arange(K)[None, :] >= st["nk"][:, None]
    assert np.all(slots[:, pad] == 0.0) and np.array_equal(slots[:, ~pad], st["slots"][:, ~pad])
    assert np.all(own[:, ~st["own_mask"]] == 0.0) and np.array_equal(own[:, st["own_mask"]], st["own"][:, st["own_mask"]])
    # the transpose: a stable sort by column, ties in (case, entry) order
    trows = R.transpose_rows(rows, npoints)
    for c, tr in enumerate(trows):
        assert [i for i, _ in tr] == sorted(i for i, _ in tr)
    tm = R.pack(trows, nop)
    assert op.fill_transposed is None
    assert op.prepare_transpose() is True and op.prepare_transpose() is False
    for k in ("len", "width", "soff", "col"):
        assert np.array_equal(op._t[k].numpy(), tm[k]), k
    assert np.array_equal(op._tval.numpy(), tm["val"])
    assert op.fill_transposed == sum(len(r) for r in rows) / max(len(tm["col"]), 1) or len(tm["col"]) == 0
    # CSR: sorted columns, duplicates summed
    csr = op.to_sparse_csr(1)
    want, tol = R.dense_bound(rows, npoints, 1)
    assert tuple(csr.shape) == (nrows, npoints)
    got = csr.to_dense().numpy()
    assert np.all(np.abs(got - want) <= tol)
    assert op.memory_used() > 0
    op.close()
    with pytest.raises(RuntimeError, match="closed"):
        op.coefficients()


def test_exact_row_sum_and_the_gamma_bound():
    """Any fp64 summation of a row, in any order, fused or not, is within gamma_n sum |val x| of the exact sum, n = len + 1."""
    st = R.random_structure(65, 80, 66, 2, seed=2, empty_slice=False)
    rows = R.rows_of(st["hoods"], st["nk"], st["slots"], st["own"], st["own_mask"], st["pts"])
    rng = np.random.default_rng(3)
    X = rng.standard_normal((2, 80)) * 10.0 ** rng.integers(-3, 4, (2, 80))
    exact, mag = R.exact_apply(rows, X, 2)
    lens = np.array([len(r) for r in rows])
    assert lens.min() == 0 and lens.max() >= 66
    assert R.gamma(1) == 2.0 ** -53 / (1 - 2.0 ** -53)
    for i, row in enumerate(rows):
        for r in range(2):
            for o in range(2):
                terms = [v[o] * X[r, c] for c, v in row]
                fwd = 0.0
                for t in terms:
                    fwd += t
                bwd = 0.0
                for t in reversed(terms):
                    bwd += t
                for got in (fwd, bwd, float(np.sum(terms)) if terms else 0.0):
                    assert abs(got - exact[r, o, i]) <= R.gamma(lens[i] + 1) * mag[r, o, i]
        if not row:
            assert np.all(exact[:, :, i] == 0.0) and np.all(mag[:, :, i] == 0.0)


def test_stencil_rows_against_the_defs_constants():
    import wlsqm
    import wlsqm.hip as h
    nd = P._NDOF
    for dim, axes in ((1, "X"), (2, "XY"), (3, "XYZ")):
        idx = lambda name: getattr(wlsqm, "i%d_%s" % (dim, name))
        for order in (2, 3, 4):
            no = nd[dim][order]
            rows = h.stencil_rows(dim, order, "value", "gradient", "laplacian", idx(axes[-1] + "2")).numpy()
            assert rows.shape == (3 + dim, no) and rows.dtype == np.float64
            want = np.zeros((3 + dim, no))
            want[0, idx("F")] = 1
            for m, a in enumerate(axes):
                want[1 + m, idx(a)] = 1
                want[1 + dim, idx(a + "2")] = 1
            want[2 + dim, idx(axes[-1] + "2")] = 1
            assert np.array_equal(rows, want)
        assert h.stencil_rows(dim, 0, "value").shape == (1, 1)
        assert h.stencil_rows(dim, 1, "gradient").shape == (dim, nd[dim][1])
        for order, what in ((0, "gradient"), (1, "laplacian"), (2, nd[dim][2]), (3, idx("X4"))):
            with pytest.raises(ValueError, match="needs a fit of order"):
                h.stencil_rows(dim, order, what)
        for what in ("hessian", 1.5, True, nd[dim][4], -1):
            with pytest.raises(ValueError):
                h.stencil_rows(dim, 4, what)
        with pytest.raises(ValueError):
            h.stencil_rows(dim, 2)
    with pytest.raises(ValueError):
        h.stencil_rows(4, 2, "value")
    with pytest.raises(ValueError):
        h.stencil_rows(2, 5, "value")


class _ReachedTheLibrary(BaseException):
    pass


def _raises(message, fn, *args, **kw):
    """fn raises ValueError / RuntimeError matching `message` before the library is reached."""
    from wlsqm import _binding

    def no_library():
        raise _ReachedTheLibrary()

    real = _binding.lib
    _binding.lib = no_library
    try:
        with pytest.raises((ValueError, RuntimeError), match=message):
            fn(*args, **kw)
    finally:
        _binding.lib = real


def test_argument_checks_need_no_device():
    import wlsqm.hip as h
    D = OnDevice
    f64 = torch.float64
    n, K, npoints, no = 4, 7, 10, 6
    geo = dict(S=torch.rand((npoints, 2), dtype=f64), hoods=torch.ones((n, K), dtype=torch.int32), nk=torch.full((n,), K, dtype=torch.int32),
               knowns=torch.zeros((n,), dtype=torch.int64), weighting_method=torch.full((n,), 2, dtype=torch.int32),
               rows=torch.ones((2, no), dtype=f64))

    def make(order=2, dim=2, **spoilt):
        a = {k: D(v) for k, v in geo.items()}
        a.update(spoilt)
        return h.StencilOperator(dim, order, **a)

    _raises("expected 'int32'.*argument hoods", make, hoods=D(geo["hoods"].long()))
    _raises("must be a device", make, S=geo["S"])
    _raises("must be contiguous", make, S=D(geo["S"].t().contiguous().t()))
    _raises("fewer than the 4 cases", make, nk=D(geo["nk"][:3]))
    _raises("rows must be \\(nop, no\\) or \\(nop, ncases, no\\)", make, rows=D(geo["rows"][0]))
    _raises("expected 'float64'.*argument rows", make, rows=D(geo["rows"].float()))
    _raises("rows has 5 columns, need at least number_of_dofs\\(2, 2\\) = 6", make, rows=D(geo["rows"][:, :5]))
    _raises("rows has 3 rows, fewer than the 4 cases", make, rows=D(torch.ones((2, 3, no), dtype=f64)))
    _raises("not contiguous in the same dimension. \\(argument rows\\)", make, rows=D(torch.ones((2, 2 * no), dtype=f64)[:, ::2]))
    _raises("rows has 0 rows", make, rows=D(geo["rows"][:0]))
    _raises("integer order", make, order=D(geo["nk"]))
    _raises("order must be", make, order=5)
    _raises("unsupported \\(dimension, order\\)", make, dim=3, order=3, S=D(torch.rand((npoints, 3), dtype=f64)),
            rows=D(torch.ones((1, 20), dtype=f64)))
    _raises("expected 'int32'.*argument point_index", make, point_index=D(torch.arange(n)))

    co = dict(hoods=geo["hoods"], nk=geo["nk"], slots=torch.zeros((2, n, K), dtype=f64))
    fc = lambda **spoilt: h.StencilOperator.from_coefficients(npoints=npoints, **dict({k: D(v) for k, v in co.items()}, **spoilt))
    _raises("slots must be at least \\(nop, ncases, 7\\)", fc, slots=D(co["slots"][:, :, :6]))
    _raises("wrong number of dimensions.*argument slots", fc, slots=D(co["slots"][0]))
    _raises("own and own_mask go together", fc, own=D(torch.zeros((2, n), dtype=f64)))
    _raises("expected 'bool'.*argument own_mask", fc, own=D(torch.zeros((2, n), dtype=f64)), own_mask=D(torch.zeros(n, dtype=torch.int32)))
    _raises("expected 'int32'.*argument nk", fc, nk=D(co["nk"].long()))

    # an operator without device state: what the checks of its methods look at
    op = h.StencilOperator.__new__(h.StencilOperator)
    op._m, op._t, op._tval = dict(total=0), None, None
    op.nop, op.ncases, op.npoints, op.K, op.no, op._device = 2, n, npoints, K, no, torch.device("cpu")
    op.known_coef, op.has_known_derivatives = None, False
    F, g = torch.zeros(npoints, dtype=f64), torch.zeros((2, n), dtype=f64)
    for call in (op.apply, lambda F_, **kw: h.differentiable_stencil_apply(op, F_, **kw)):
        _raises("expected 'float64'.*argument F", call, D(F.float()))
        _raises("must be a device", call, F)
        _raises("must be a device", call, np.zeros(npoints))
        _raises("wrong number of dimensions.*argument F", call, D(torch.zeros((1, 1, npoints), dtype=f64)))
        _raises("F has fewer entries than S has points", call, D(F[:-1]))
        _raises("F has 0 rows", call, D(torch.zeros((0, npoints), dtype=f64)))
    op.has_known_derivatives, op.known_coef = True, torch.zeros((2, n, no), dtype=f64)
    _raises("pass known=", op.apply, D(F))
    _raises("pass known=", h.differentiable_stencil_apply, op, D(F))
    _raises("known has 5 columns", op.apply, D(F), known=D(torch.zeros((n, 5), dtype=f64)))
    _raises("known has 3 rows", op.apply, D(F), known=D(torch.zeros((3, no), dtype=f64)))
    _raises("known is a stack of 2, F one field", op.apply, D(F), known=D(torch.zeros((2, n, no), dtype=f64)))
    op.has_known_derivatives = False
    _raises("out must be a float64 device tensor of shape \\(2, 4\\)", op.apply, D(F), out=D(torch.zeros((2, 5), dtype=f64)))
    _raises("expected 'float64'.*argument out", op.apply, D(F), out=D(torch.zeros((2, n))))
    both = torch.zeros(npoints + 2 * n, dtype=f64)
    _raises("overlaps", op.apply, D(both[:npoints]), out=D(both[npoints - 1:npoints - 1 + 2 * n].view(2, n)))
    _raises("g must be \\(nop, ncases\\) = \\(2, 4\\)", op.apply_transpose, D(g[:, :3]))
    _raises("expected 'float64'.*argument g", op.apply_transpose, D(g.float()))
    _raises("must be a device", op.apply_transpose, g)
    _raises("out must be a float64 device tensor of shape \\(10,\\)", op.apply_transpose, D(g), out=D(torch.zeros(9, dtype=f64)))
    _raises("the operator has 2 value planes", op.to_sparse_csr, 2)
    op.close()
    for call in (lambda: op.apply(D(F)), lambda: op.apply_transpose(D(g)), op.prepare_transpose, op.coefficients, op.to_sparse_csr,
                 op.memory_used, lambda: op.fill, lambda: h.differentiable_stencil_apply(op, D(F))):
        _raises("the stencil operator has been closed", call)


def test_header_binding_and_library_name_the_entry_point():
    import os
    import subprocess
    from wlsqm import _binding
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "wlsqm_hip.h")).read()
    assert "int wlsqm_hip_sell_apply_device(" in header and "soff[i / 64] + 64 * e + i % 64" in header
    assert "wlsqm_hip_sell_apply_device" in open(os.path.join(root, "python-wlsqm_amd", "wlsqm", "_binding.py")).read()
    if os.path.exists(_binding.LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", _binding.LIB_PATH], capture_output=True, text=True).stdout
        assert " T wlsqm_hip_sell_apply_device" in syms


MASKS = (0, 1, 3)              # no knowns, b_F, b_F | b_X


@pytest.mark.parametrize("family", ("plain", "grid", "aniso"))
def test_the_algebra_in_mpmath(family):
    """For knowns masks 0, b_F and b_F | b_X: the stencil that the transposed operator gives for a row lambda — c_k on neighbour k, the
    own coefficient on the point's value (F known), known_coef on the other known DOFs — applied to the data equals lambda . fi_out of
    the fit, to 1e-40 relative in mpmath; and truth_adjoint_mp is that stencil rounded once."""
    from mpmath import mp, mpf
    dim, order, K, n = 2, 2, 32, 6
    b = A.make(family, dim, order, K, n)
    no = b["no"]
    kn = np.array([MASKS[j % 3] for j in range(n)], np.int64)
    wm = np.array([2, 2, 2, 1, 1, 1], np.int32)
    lam = np.random.default_rng(5).uniform(-1, 1, (n, no))
    op = P.truth_operator_mp(dim, b["xk"], b["nk"], b["xi"], b["order_a"], kn, wm, as_mp=True)
    fi, _ = P.truth_fit_mp(dim, b["xk"], b["fk"], b["nk"], b["xi"], b["fi0"], b["order_a"], kn, wm, as_mp=True)
    gfk, gfi, _ = P.truth_adjoint_mp(op, lam)
    with mp.workdps(60):
        for j in range(n):
            lm = [mpf(float(v)) for v in lam[j]]
            U = [a for a in range(no) if op.kind[j, a] == P.DOF_UNKNOWN]
            Kn = [a for a in range(no) if op.kind[j, a] == P.DOF_KNOWN]
            assert Kn == [a for a in range(no) if (MASKS[j % 3] >> a) & 1]
            c = [mp.fsum(op.S[j, k, a] * lm[a] for a in U) for k in range(int(b["nk"][j]))]
            coef = {bk: lm[bk] + mp.fsum(lm[a] * op.J[j, a, bk] for a in U) for bk in Kn}
            stencil = mp.fsum(c[k] * mpf(float(b["fk"][j, k])) for k in range(len(c)))
            stencil += mp.fsum(coef[bk] * mpf(float(b["fi0"][j, bk])) for bk in Kn)       # bk = 0: the own entry of the matrix
            want = mp.fsum(lm[a] * fi[j, a] for a in range(no))
            scale = mp.fsum(abs(lm[a] * fi[j, a]) for a in range(no))
            assert abs(stencil - want) <= mpf(10) ** -40 * scale, (family, j)
            assert np.array_equal(gfk[j, :len(c)], [float(v) for v in c]) and np.all(gfk[j, len(c):] == 0.0)
            for a in range(no):
                assert gfi[j, a] == (float(coef[a]) if a in Kn else 0.0)
