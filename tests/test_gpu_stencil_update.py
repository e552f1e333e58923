"""GPU tests of StencilOperator.update (the fused build kernel "stencil-build" of csrc/fit_adjoint.hip and the permute kernel of
csrc/stencil.hip).

  1. an update is the constructor on the new geometry: coefficients, known_coef and apply bit for bit, for the systems up to 10 unknowns;
  2. the 15-unknown shape against the mpmath truth of the fit, the reference being the constructor's operator on the same geometry;
  3. new neighbour lists; 4. the transposed refresh; 5. what the kernel never writes; 6. graph capture; 7. errors.
The reference of 1 - 4 is the constructor (one adjoint launch per operator, scatter, pack): not the code under test.
"""
import ctypes as C

import numpy as np
import pytest

import _adversarial as A
import _parity as P
from _device_helpers import bits, dev as _t, nan as _nan, same_bits as _same_bits, wlsqm  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

N = A.N_OP
WORKERS = 12
BITWISE = ((1, 2, 8), (2, 2, 32), (3, 2, 40), (2, 3, 24))      # (2, 3, 24): 10 unknowns, the edge of pin_fma
# the other systems up to 10 unknowns: whether the own entry's sum is fused follows the adjoint kernel's compiled code, shape by shape
OTHERS = ((1, 0, 8), (1, 1, 8), (1, 3, 8), (1, 4, 12), (2, 0, 32), (2, 1, 32), (3, 0, 40), (3, 1, 40))
BIG = (2, 4, 64)                                                # 15 unknowns: held to the truth, not to the adjoint's bits
EDGES = ("tiny_edge", "huge_edge")                              # reported, not asserted (as tests/test_gpu_stencil.py)
# the families of test 2: those whose truths (15 unknowns, 64 neighbours, 96 cases each) the worker pool returns within seconds
BIG_FAMILIES = ("plain", "aniso", "onesided", "lattice") + EDGES
_ids = lambda s: "%dD-o%d-K%d" % s


def _table(f, dim, order, K, n=N):
    """The batch of a family as an index-based problem through A.point_table: every family has the same hoods and point_index."""
    b = A.op_batch(f, dim, order, K, n)
    S, F, hoods, pidx = A.point_table(b)
    return b, S, F, hoods, pidx


def _frame(dim, order, K, n=N):
    """What geometry A and every geometry B share: ragged nk with 0 and K, the padding of hoods pointing outside the table, masks 0, b_F,
    b_F | b_X, stray high bits and one case with every DOF known."""
    b, S, F, hoods, pidx = _table("plain", dim, order, K, n)
    no, npoints = b["no"], len(F)
    rng = np.random.default_rng([dim, order, K, n])
    nk = rng.integers(no, K + 1, n).astype(np.int32)
    nk[0], nk[1], nk[2] = 0, K, K
    hoods = hoods.copy()
    pad = np.arange(K)[None, :] >= nk[:, None]
    hoods[pad] = np.where((np.arange(n)[:, None] + np.arange(K)[None, :]) % 2 == 0, -1, npoints)[pad]
    kn = b["kn"].copy()
    kn[5::7] = 3                                                    # b_F | b_X: a known derivative
    kn[10] = 1 << 40                                                # a stray high bit: the last DOF drops out
    kn[40] = (1 << 40) | 1                                          # the same beside b_F
    kn[12] = kn[60] = (1 << no) - 1                                 # every DOF known
    return dict(no=no, npoints=npoints, nk=nk, kn=kn, wm=b["wm"], hoods=hoods, pidx=pidx, pad=pad, S=S, F=F, rng=rng)


def _poison(op):
    """A's values only have to be overwritten: NaN in every value plane and in known_coef shows an entry that an update left alone."""
    op._val.fill_(float("nan"))
    op.known_coef.fill_(float("nan"))


def _same_operator(op, want, F, known, what):
    for got, ref in zip(op.coefficients(), want.coefficients()):
        assert _same_bits(got.cpu().numpy(), ref.cpu().numpy()), what
    assert _same_bits(op.known_coef.cpu().numpy(), want.known_coef.cpu().numpy()), what
    assert _same_bits(op.apply(F, known=known).cpu().numpy(), want.apply(F, known=known).cpu().numpy()), what


# ---- 1. an update is the constructor on the new geometry ---------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", BITWISE, ids=_ids)
def test_update_is_the_constructor_on_the_new_geometry(wlsqm, shape):
    _constructor_on_the_new_geometry(shape, (1, 3, 5))


@pytest.mark.parametrize("shape", OTHERS, ids=_ids)
def test_the_other_systems_up_to_ten_unknowns(wlsqm, shape):
    _constructor_on_the_new_geometry(shape, (3,))


def _constructor_on_the_new_geometry(shape, nops):
    import torch
    import wlsqm.hip as whip
    dim, order, K = shape
    fr = _frame(dim, order, K)
    no, rng = fr["no"], fr["rng"]
    idx = (_t(fr["hoods"]), _t(fr["nk"]), _t(fr["kn"]), _t(fr["wm"]))
    pidx = _t(fr["pidx"])
    known = _t(rng.uniform(-1, 1, (N, no)))
    tables = {f: _table(f, dim, order, K)[1:3] for f in A.OP_FAMILIES}
    seen = {}
    for nop in nops:                                                    # 5 crosses the block edge of every shape (4 or 2 operators per block)
        for rows in (rng.uniform(-1, 1, (5, no))[:nop], rng.uniform(-1, 1, (5, N, no))[:nop]):
            rows = _t(rows)
            op = whip.StencilOperator(dim, order, _t(fr["S"]), *idx, rows, point_index=pidx)
            for f in A.OP_FAMILIES:
                S, F = (_t(x) for x in tables[f])
                want = whip.StencilOperator(dim, order, S, *idx, rows, point_index=pidx)
                assert want.has_known_derivatives
                _poison(op)
                assert op.update(S) is op and whip.last_kernel() == "stencil-build"
                assert op.has_known_derivatives is True
                _same_operator(op, want, F, known, (shape, f, nop, rows.dim()))
                want.close()
            op.close()
    # a result does not depend on its block: operator 0 of the shared rows alone, first of three and first of five is one set of bits
    rows = _t(rng.uniform(-1, 1, (5, no)))
    S = _t(tables["aniso"][0])
    for nop in (1, 3, 5):
        op = whip.StencilOperator(dim, order, _t(fr["S"]), *idx, rows[:nop], point_index=pidx)
        _poison(op)
        op.update(S)
        slots, own = (x.cpu().numpy() for x in op.coefficients())
        kc = op.known_coef.cpu().numpy()
        for o in range(nop):
            for name, x in (("slots", slots[o]), ("own", own[o]), ("kc", kc[o])):
                assert _same_bits(seen.setdefault((o, name), x), x), (shape, nop, o, name)
        op.close()
    torch.cuda.synchronize()


def test_three_slices_and_new_rows(wlsqm):
    """130 rows: two full slices and a third of two rows; rows= replaces the operators, of either form."""
    import wlsqm.hip as whip
    dim, order, K, n = 2, 2, 32, 130
    fr = _frame(dim, order, K, n)
    no, rng = fr["no"], fr["rng"]
    idx = (_t(fr["hoods"]), _t(fr["nk"]), _t(fr["kn"]), _t(fr["wm"]))
    pidx = _t(fr["pidx"])
    known = _t(rng.uniform(-1, 1, (n, no)))
    _, S, F, _, _ = _table("onesided", dim, order, K, n)
    S, F = _t(S), _t(F)
    for shape in ((3, no), (3, n, no)):
        rows, rows2 = _t(rng.uniform(-1, 1, shape)), _t(rng.uniform(-1, 1, shape))
        op = whip.StencilOperator(dim, order, _t(fr["S"]), *idx, rows, point_index=pidx)
        assert op._m["width"].shape[0] == 3
        _poison(op)
        op.update(S)
        want = whip.StencilOperator(dim, order, S, *idx, rows, point_index=pidx)
        _same_operator(op, want, F, known, ("rows", shape))
        _poison(op)
        op.update(S, rows=rows2)
        want2 = whip.StencilOperator(dim, order, S, *idx, rows2, point_index=pidx)
        _same_operator(op, want2, F, known, ("rows2", shape))
        _poison(op)
        op.update(S)                                                    # the operators stay replaced
        _same_operator(op, want2, F, known, ("rows2 kept", shape))
        for o in (op, want, want2):
            o.close()


# ---- 2. the 15-unknown shape against the truth ---------------------------------------------------------------------------------------------

def _big_truths():
    dim, order, K = BIG
    step = 16
    per = N // step
    res = A.truths([(f, dim, order, K, N, lo, lo + step) for f in BIG_FAMILIES for lo in range(0, N, step)], WORKERS)
    return {f: (np.concatenate([r[0] for r in res[i * per:(i + 1) * per]]), np.concatenate([r[1] for r in res[i * per:(i + 1) * per]]))
            for i, f in enumerate(BIG_FAMILIES)}


def test_fifteen_unknowns_against_the_mpmath_truth(wlsqm):
    """rows = the identity: after update(S_f), apply(F)[a, j] is DOF a of the fit of case j.  The reference is apply of the constructor's
    operator on the same geometry; per case and DOF the scale is s = sum_k |c_k F_k| (the own entry included) of that operator."""
    import torch
    import wlsqm.hip as whip
    dim, order, K = BIG
    truths = _big_truths()
    eps = np.finfo(np.float64).eps
    eye = torch.eye(15, dtype=torch.float64, device="cuda")
    op = None
    for f in BIG_FAMILIES:
        b = A.op_batch(f, dim, order, K)
        if f == "lattice":                                               # a real lattice: its own table and index arrays, an operator of its own
            S, F, hoods, pidx = b["S"], b["F"], b["hoods"], b["pidx"]
        else:
            S, F, hoods, pidx = A.point_table(b)
        nk, kn = b["nk"], b["kn"]
        geo = (_t(hoods), _t(nk), _t(kn), _t(b["wm"]))
        want = whip.StencilOperator(dim, order, _t(S), *geo, eye, point_index=_t(pidx))
        if op is None or f == "lattice":
            # geometry A: the same index arrays on a table that is not this family's (here: stretched and moved)
            mine = whip.StencilOperator(dim, order, _t(S) * 1.25 + 0.5, *geo, eye, point_index=_t(pidx))
            if f != "lattice":
                op = mine
        else:
            mine = op
        _poison(mine)
        mine.update(_t(S))
        assert whip.last_kernel() == "stencil-build" and not mine.has_known_derivatives, f
        got = mine.apply(_t(F)).cpu().numpy().T
        ref = want.apply(_t(F)).cpu().numpy().T
        slots, own = (x.cpu().numpy() for x in want.coefficients())
        live = np.arange(K)[None, :] < nk[:, None]
        Fk = np.where(live, F[np.where(live, hoods, 0)], 0.0)
        s = (np.einsum("ajk,jk->ja", np.abs(slots), np.abs(Fk)) + np.abs(own).T * np.abs(F[pidx])[:, None])
        s[s == 0] = 1.0
        T, kappa = truths[f]

        def err(x, y):
            with np.errstate(invalid="ignore", over="ignore"):
                e = (np.abs(x - y) / s).max(axis=1)
            return np.where(np.isfinite(e), e, np.inf)

        e_cr, e_ct, e_rt = err(got, ref), err(got, T), err(ref, T)
        qc, qr = e_ct / (eps * kappa ** 2), e_rt / (eps * kappa ** 2)
        what = "stencil update + apply, %s %dD order %d K %d" % (f, dim, order, K)
        print("%-60s err: gpu-truth %.3g ref-truth %.3g gpu-ref %.3g   max q: gpu %.3g ref %.3g" % (what, e_ct.max(), e_rt.max(), e_cr.max(),
                                                                                                 qc.max(), qr.max()))
        if f not in EDGES:
            P.assert_scaled(e_cr, e_ct, e_rt, what)
            P.assert_q(qc, qr, kappa, what)
        want.close()
        if mine is not op:
            mine.close()
    op.close()


# ---- 3. new neighbour lists, 4. the transposed refresh -----------------------------------------------------------------------------------

def _permuted(hoods, nk, rng):
    h2 = hoods.copy()
    for j in range(len(nk)):
        h2[j, :nk[j]] = rng.permutation(hoods[j, :nk[j]])
    return h2


@pytest.mark.parametrize("shape", ((2, 2, 32), (3, 2, 40)), ids=_ids)
def test_new_neighbour_lists(wlsqm, shape):
    import torch
    import wlsqm.hip as whip
    dim, order, K = shape
    fr = _frame(dim, order, K)
    no, rng = fr["no"], fr["rng"]
    rest = (_t(fr["nk"]), _t(fr["kn"]), _t(fr["wm"]))
    pidx = _t(fr["pidx"])
    rows = _t(rng.uniform(-1, 1, (3, no)))
    _, S, F, _, _ = _table("collinear", dim, order, K)
    S, F, known = _t(S), _t(F), _t(rng.uniform(-1, 1, (N, no)))
    h2 = _permuted(fr["hoods"], fr["nk"], rng)
    assert not np.array_equal(h2, fr["hoods"])
    op = whip.StencilOperator(dim, order, _t(fr["S"]), _t(fr["hoods"]), *rest, rows, point_index=pidx)
    assert op.prepare_transpose() is True and op.fill_transposed is not None
    want = whip.StencilOperator(dim, order, S, _t(h2), *rest, rows, point_index=pidx)
    _poison(op)
    op._m["col"][op._entries()[0]] = -7                                 # every live column must be rewritten
    op.update(S, hoods=_t(h2))
    assert whip.last_kernel() == "stencil-build" and op.fill_transposed is None
    assert torch.equal(op._m["col"], want._m["col"])
    _same_operator(op, want, F, known, shape)
    g = _t(rng.standard_normal((3, N)))
    assert torch.equal(bits(op.apply_transpose(g)), bits(want.apply_transpose(g)))      # rebuilt for the new columns
    assert op.fill_transposed == want.fill_transposed
    _poison(op)
    op.update(S)                                                        # the new lists are the operator's from now on
    _same_operator(op, want, F, known, shape)
    for bad in (h2[:, :K - 1], h2[:N - 1], np.concatenate([h2, h2[:, :1]], axis=1)):
        with pytest.raises(ValueError, match="another shape needs a new operator"):
            op.update(S, hoods=_t(bad))
    op.close(); want.close()


def test_transposed_refresh(wlsqm):
    import torch
    import wlsqm.hip as whip
    dim, order, K = 2, 2, 32
    fr = _frame(dim, order, K)
    no, rng = fr["no"], fr["rng"]
    idx = (_t(fr["hoods"]), _t(fr["nk"]), _t(fr["kn"]), _t(fr["wm"]))
    pidx = _t(fr["pidx"])
    rows = _t(rng.uniform(-1, 1, (3, no)))
    S = _t(_table("aniso", dim, order, K)[1])
    op = whip.StencilOperator(dim, order, _t(fr["S"]), *idx, rows, point_index=pidx)
    want = whip.StencilOperator(dim, order, S, *idx, rows, point_index=pidx)
    assert op.prepare_transpose() is True
    fill, used = op.fill_transposed, op.memory_used()
    assert used >= 8 * op._nnz and op._tpair.dtype == torch.int32 and tuple(op._tpair.shape) == (2, op._nnz)
    _poison(op)
    op._tval.fill_(float("nan"))
    op.update(S)
    assert whip.last_kernel() == "stencil-permute"
    g = _t(rng.standard_normal((2, 3, N)))
    assert torch.equal(bits(op.apply_transpose(g)), bits(want.apply_transpose(g)))
    assert op.fill_transposed == fill and op.memory_used() == used and op.prepare_transpose() is False
    assert _same_bits(op._tval.cpu().numpy()[:, op._tpair[0].long().cpu().numpy()], want._tval.cpu().numpy()[:, op._tpair[0].long().cpu().numpy()])
    op.close(); want.close()


# ---- 5. what is never written ----------------------------------------------------------------------------------------------------------------

def test_what_the_kernel_never_writes(wlsqm):
    """wlsqm_hip_stencil_build_device on arrays the test owns: a frame with a slice wider than some of its rows and one empty slice; every
    live entry is written, every other element keeps its sentinel; with len one shorter than the geometry says, nothing at or beyond len."""
    import torch
    from wlsqm import _binding
    dim, order, K, n, nop = 2, 2, 12, 130, 3
    no = 6
    rng = np.random.default_rng(51)
    b, S, F, hoods, pidx = _table("plain", dim, order, K, n)
    npoints = len(F)
    nk = rng.integers(no, K + 1, n).astype(np.int32)
    nk[3], nk[7] = K + 5, -2                                            # clamped to K and to 0
    kn = np.where(np.arange(n) % 3 == 0, 1, 0).astype(np.int64)
    kn[9], kn[20] = 63, 3
    nk[64:128], kn[64:128] = 0, 0                                       # the second slice is empty
    kn[7] = 1                                                           # a row of the own entry alone
    nkc = np.clip(nk, 0, K)
    hoods = hoods.copy()
    hoods[np.arange(K)[None, :] >= nkc[:, None]] = npoints + 12345      # never dereferenced
    rows = rng.uniform(-1, 1, (nop, n, no))

    def run(lens):
        ns = (n + 63) // 64
        padded = np.zeros(ns * 64, np.int64); padded[:n] = lens
        width = padded.reshape(ns, 64).max(axis=1)
        soff = np.concatenate([[0], np.cumsum(64 * width)]).astype(np.int64)
        total = int(soff[-1])
        col = torch.full((total + 64,), -7, dtype=torch.int32, device="cuda")          # 64 more: a write past the end would show
        val = _nan(nop, total + 64)
        kc = _nan(nop, n, no + 1)
        d = dict(S=_t(S), hoods=_t(hoods), pidx=_t(pidx), nk=_t(nk), kn=_t(kn), wm=_t(b["wm"]), rows=_t(rows), len=_t(lens.astype(np.int32)),
                 soff=_t(soff))
        p = lambda t: C.c_void_p(t.data_ptr())
        rc = _binding.lib().wlsqm_hip_stencil_build_device(dim, order, n, K, p(d["S"]), p(d["hoods"]), K, p(d["pidx"]), p(d["nk"]), p(d["kn"]),
                                                           p(d["wm"]), p(d["rows"]), n * no, no, nop, p(d["len"]), p(d["soff"]), p(col), p(val),
                                                           total + 64, p(kc), n * (no + 1), no + 1, 0, None)
        assert rc == 0
        torch.cuda.synchronize()
        j = np.arange(n)
        e = np.arange(K + 1)
        pos = (soff[j // 64] + j % 64)[:, None] + 64 * e[None, :]
        return col.cpu().numpy(), val.cpu().numpy(), kc.cpu().numpy(), pos, width, total

    fbit = (kn & 1).astype(np.int64)
    lens = nkc + fbit
    col, val, kc, pos, width, total = run(lens)
    assert width[1] == 0 and width[0] > lens[:64].min() and total > lens.sum()
    live = np.arange(K + 1)[None, :] < lens[:, None]
    written = np.zeros(total + 64, bool)
    written[pos[live]] = True
    assert np.all(col[~written] == -7) and np.all(np.isnan(val[:, ~written]))
    assert np.all(col[written] != -7) and not np.isnan(val[:, written]).any()
    nb = np.arange(K)[None, :] < nkc[:, None]
    assert np.array_equal(col[pos[:, :K][nb]], hoods[nb])
    own = fbit == 1
    assert np.array_equal(col[pos[np.arange(n), nkc][own]], pidx[own])
    assert not np.isnan(kc[:, :, :no]).any() and np.all(np.isnan(kc[:, :, no]))
    # len one shorter on a few rows (and longer than the geometry on one): nothing at or beyond len, nothing beyond the row's own entries
    short = lens.copy()
    cut = np.array([0, 5, 9, 63, 128])
    short[cut] -= 1
    short[1] += 1
    assert short[cut].min() >= 0
    col2, val2, _, pos2, _, total2 = run(short)
    may = np.arange(K + 1)[None, :] < np.minimum(short, lens)[:, None]
    written2 = np.zeros(total2 + 64, bool)
    written2[pos2[may]] = True
    assert np.all(col2[~written2] == -7) and np.all(np.isnan(val2[:, ~written2]))
    assert np.all(col2[written2] != -7) and not np.isnan(val2[:, written2]).any()
    # ncases == 0 launches nothing
    assert _binding.lib().wlsqm_hip_stencil_build_device(dim, order, 0, K, None, None, K, None, None, None, None, None, 0, 0, 1, None, None, None,
                                                         None, 0, None, 0, 0, 0, None) == 0


# ---- 6. capture --------------------------------------------------------------------------------------------------------------------------------

def test_capture(wlsqm):
    import torch
    import wlsqm.hip as whip
    dim, order, K = 2, 2, 32
    b, SA, F, hoods, pidx = _table("plain", dim, order, K)
    SB = _table("aniso", dim, order, K)[1]
    kn = np.where(np.arange(N) % 2 == 0, 1, 0).astype(np.int64)         # F known or nothing: no known derivatives
    geo = (_t(hoods), _t(b["nk"]), _t(kn), _t(b["wm"]))
    rows = whip.stencil_rows(dim, order, "gradient", "laplacian", device="cuda")
    S, F = _t(SA), _t(F)
    op = whip.StencilOperator(dim, order, S, *geo, rows, point_index=_t(pidx))
    Y = _nan(3, N)

    def step():
        op.update(S, check=False)
        op.apply(F, out=Y)

    step()                                                               # warm-up outside the capture
    torch.cuda.synchronize()
    assert not op.has_known_derivatives
    at_a = Y.clone()
    S.copy_(_t(SB))
    before = torch.cuda.memory_allocated()
    op.update(S, check=False)
    assert torch.cuda.memory_allocated() == before                       # kernels only: nothing allocated
    op.apply(F, out=Y)
    torch.cuda.synchronize()
    eager = Y.clone()
    assert not torch.equal(bits(eager), bits(at_a))
    S.copy_(_t(SA))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        step()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(Y), bits(at_a))
    S.copy_(_t(SB))
    Y.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(Y), bits(eager))
    refused = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="pass check=False inside the capture"):
        with torch.cuda.graph(refused, stream=torch.cuda.Stream()):
            op.update(S)
    torch.cuda.synchronize()
    op.update(S)                                                         # the capture ended cleanly: the operator and the stream work on
    assert torch.equal(bits(op.apply(F)), bits(eager))
    op.close()


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------------------

def test_errors(wlsqm):
    import torch
    import wlsqm.hip as whip
    dim, order, K = 2, 2, 32
    b, S, F, hoods, pidx = _table("plain", dim, order, K)
    npoints, no = len(F), b["no"]
    nk = b["nk"].copy()
    nk[4] = K - 3
    geo = (_t(nk), _t(b["kn"]), _t(b["wm"]))
    rows = _t(np.ones((2, no)))
    S = _t(S)
    op = whip.StencilOperator(dim, order, S, _t(hoods), *geo, rows, point_index=_t(pidx))
    before = [x.clone() for x in op.coefficients()]
    bad = hoods.copy()
    bad[4, K - 4] = npoints                                             # a live index one past the table
    with pytest.raises(ValueError, match="a live entry names a point outside 0 .. npoints - 1 = %d" % (npoints - 1)):
        op.update(S, hoods=_t(bad))
    for x, y in zip(before, op.coefficients()):                         # refused before anything was enqueued
        assert torch.equal(bits(x), bits(y))
    ok = hoods.copy()
    ok[4, K - 3:] = npoints                                             # the padding may name anything
    op.update(S, hoods=_t(ok))
    with pytest.raises(ValueError, match="S has fewer points"):
        op.update(S[:npoints - 1])
    with pytest.raises(ValueError, match="expected 'float64'.*argument S"):
        op.update(S.float())
    with pytest.raises(ValueError, match="must be contiguous"):
        op.update(torch.cat([S, S], dim=1)[:, :2])
    with pytest.raises(ValueError, match="must be a device"):
        op.update(S.cpu())
    with pytest.raises(ValueError, match="expected 'int32'.*argument hoods"):
        op.update(S, hoods=_t(hoods.astype(np.int64)))
    with pytest.raises(ValueError, match="same device"):
        op.update(S, hoods=_FakeDevice(_t(hoods)))
    with pytest.raises(ValueError, match="rows must keep the operator's form"):
        op.update(S, rows=_t(np.ones((3, no))))
    with pytest.raises(ValueError, match="rows must keep the operator's form"):
        op.update(S, rows=_t(np.ones((2, N, no))))
    with pytest.raises(ValueError, match="expected 'float64'.*argument rows"):
        op.update(S, rows=rows.float())
    co = whip.StencilOperator.from_coefficients(_t(hoods), _t(nk), _t(np.ones((1, N, K))), npoints)
    with pytest.raises(RuntimeError, match="no fit to redo"):
        co.update(S)
    co.close()
    op.close()
    with pytest.raises(RuntimeError, match="closed"):
        op.update(S)


class _FakeDevice:
    """A device tensor that says it lives on another device."""

    def __init__(self, t):
        self._t = t

    def __getattr__(self, name):
        return getattr(self._t, name)

    @property
    def device(self):
        import torch
        return torch.device("cuda", 7)
