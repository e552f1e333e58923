"""GPU tests of the fit's geometry adjoint (csrc/fit_adjoint.hip: `geometry-adjoint-lane` / `geometry-adjoint-rows`;
wlsqm.hip.fit_many_geometry_adjoint_device, fit_cloud_geometry_adjoint_device and differentiable_fit_*(..., geometry=True)).

Truth: tests/_geometry_adjoint_ref.truth_geometry_adjoint_mp (mpmath, pinned to central differences by tests/test_geometry_adjoint_cpu.py).
Reference: geometry_adjoint_ref of the same module (fp64 numpy on the CPU oracle's fit).  Criteria, the project's own (tests/_parity.py:
NOISE_MULT, TOL, Q_FLOOR), in the case's scale s_j (the largest sum of the absolute values of the terms of one e[k][m]):
  (a) `assert_scaled`: over a family batch, the GPU's distance to the reference and to the truth within TOL + NOISE_MULT N, N the
      reference's worst distance to the truth;
  (b) `assert_q`: max_j q_j(GPU) <= NOISE_MULT max_j q_j(reference) + Q_FLOOR, q_j = err_j / (s_j eps kappa_j^2).
The GPU differentiates ITS OWN fit: fi_out comes from fit_many_device in fast mode, the reference's from the oracle.  Every family is a
batch of A.N_OP = 96 cases; the truths of a shape are computed once per module in worker processes that never touch the GPU.  The two
*_edge families are printed, not asserted (the narrowed range)."""
import os

import numpy as np
import pytest

import _adversarial as A
import _geometry_adjoint_ref as G
import _parity as P
from _device_helpers import bits as _bits, dev as _dev, nan as _nan, same_bits as _same_bits

pytestmark = pytest.mark.gpu

SWITCH = "WLSQM_HIP_ADJOINT_FORM"
N = A.N_OP
WORKERS = 12
FORMS = (("l", "geometry-adjoint-lane"), ("r", "geometry-adjoint-rows"))
_ids = lambda s: "%dD-o%d-K%d" % s


@pytest.fixture(scope="module")
def hip():
    import wlsqm.hip as h
    from wlsqm import _binding
    assert _binding.lib().wlsqm_hip_device_count() >= 1, "no HIP device: the GPU tests need a real MI355X"
    return h


class _form:
    """with _form("l") / _form("r") / _form(None): the switch of the two forms, put back on the way out."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.prev = os.environ.get(SWITCH)
        if self.value is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = self.value

    def __exit__(self, *exc):
        if self.prev is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = self.prev
        return False


_CACHE = {}


def _shape_data(shape):
    """All of A.OP_FAMILIES at one shape: the batch, g, the truth and the reference.  Computed once per module; nothing modifies it."""
    if shape in _CACHE:
        return _CACHE[shape]
    dim, order, K = shape
    truths = G.geometry_truths(shape, A.OP_FAMILIES, workers=WORKERS)
    out = {}
    for f in A.OP_FAMILIES:
        b = A.op_batch(f, dim, order, K)
        b["g"] = A.op_g(f, dim, order, K)
        b["truth"] = truths[f]
        with np.errstate(all="ignore"):
            b["ref"] = G.geometry_adjoint_ref(dim, order, b["xk"], b["fk"], b["nk"], b["xi"], b["fi0"], b["kn"], b["wm"], b["g"])
        out[f] = b
    _CACHE[shape] = out
    return out


def _forward(hip, b):
    """fi_out of the GPU's own fit in fast mode, as a device tensor."""
    fi = _dev(b["fi0"])
    hip.fit_many_device(b["dim"], b["order"], _dev(b["xk"]), _dev(b["fk"]), _dev(b["nk"]), _dev(b["xi"]), fi, _dev(b["kn"]), _dev(b["wm"]),
                        strict=False)
    return fi


def _geometry(hip, b, fi, form, want_fk=True, strided=False, n=None):
    """One explicit call with NaN-prefilled outputs under `form`; returns (grad_xk, grad_xi, grad_fk) as device tensors and the kernel."""
    import torch
    n = len(b["nk"]) if n is None else n
    K, dim = b["K"], b["dim"]
    tail = () if dim == 1 else (dim,)
    xk = _dev(b["xk"])
    if strided:
        wide = torch.zeros((n, 2 * K) + tail, dtype=torch.float64, device="cuda")
        wide[:, ::2] = xk
        xk = wide[:, ::2]
        gxk = _nan(n, 2 * K, *tail)[:, ::2]
    else:
        gxk = _nan(n, K, *tail)
    gxi = _nan(n, *tail)
    gfk = _nan(n, K) if want_fk else False
    with _form(form):
        hip.fit_many_geometry_adjoint_device(dim, b["order"], xk, _dev(b["fk"]), _dev(b["nk"]), _dev(b["xi"]), fi, _dev(b["kn"]),
                                             _dev(b["wm"]), _dev(b["g"]), grad_xk=gxk, grad_xi=gxi, grad_fk=gfk)
        kernel = hip.last_kernel()
    torch.cuda.synchronize()
    return gxk, gxi, (gfk if want_fk else None), kernel


def _flat(a, n):
    return np.asarray(a, np.float64).reshape(n, -1)


# ---- 1. every family, both forms, against the truth and the reference ----------------------------------------------------------------

@pytest.mark.parametrize("shape", G.SHAPES, ids=_ids)
def test_every_family_both_forms(hip, shape):
    dim, order, K = shape
    data = _shape_data(shape)
    for f in A.OP_FAMILIES:
        b = data[f]
        t_xk, t_xi, s, kappa = b["truth"]
        ref = b["ref"]
        fi = _forward(hip, b)
        rows = np.arange(K)[None, :] < b["nk"][:, None]
        for form, kernel in FORMS:
            gxk, gxi, gfk, ran = _geometry(hip, b, fi, form)
            assert ran == kernel, (f, form, ran)
            gxk, gxi = gxk.cpu().numpy().reshape(N, K, dim), gxi.cpu().numpy().reshape(N, dim)
            assert np.all(gxk[~rows] == 0.0), "%s %s: the padding of grad_xk is not exactly zero" % (f, shape)
            line = []
            for name, got, want, truth in (("grad_xk", _flat(gxk, N), _flat(ref["grad_xk"], N), _flat(t_xk, N)),
                                           ("grad_xi", gxi, ref["grad_xi"], t_xi)):
                what = "%s [%s], %s %dD order %d K %d" % (name, kernel, f, dim, order, K)
                with np.errstate(all="ignore"):
                    qc, qr = P.grad_q(got, truth, s, kappa), P.grad_q(want, truth, s, kappa)
                    e_cr, e_ct, e_rt = P.grad_err(got, want, s), P.grad_err(got, truth, s), P.grad_err(want, truth, s)
                line.append("%s q gpu %.3g ref %.3g, err gpu %.3g ref %.3g" % (name, qc.max(), qr.max(), e_ct.max(), e_rt.max()))
                if f in G.EDGE_FAMILIES:
                    continue                                           # reported, not asserted
                assert np.isfinite(want).all(), what + ": the reference is not finite"
                P.assert_scaled(e_cr, e_ct, e_rt, what)
                P.assert_q(qc, qr, kappa, what)
            print("%-11s %dD o%d K%2d %s  %s" % (f, dim, order, K, form, "  ".join(line)))


# ---- 2. the two forms bit for bit; the fused grad_fk against the adjoint's ------------------------------------------------------------

@pytest.mark.parametrize("shape", [s for s in G.SHAPES if A.NDOF[s[0]][s[1]] <= 10], ids=_ids)
def test_forms_agree_bit_for_bit_and_grad_fk_is_the_adjoints(hip, shape):
    import torch
    dim, order, K = shape
    data = _shape_data(shape)
    for f in G.FAMILIES:
        b = data[f]
        fi = _forward(hip, b)
        got = {form: _geometry(hip, b, fi, form) for form, _ in FORMS}
        for i in range(3):
            assert torch.equal(_bits(got["l"][i]), _bits(got["r"][i])), "%s %s: output %d differs between the forms" % (f, shape, i)
        t = {k: _dev(b[k]) for k in ("xk", "nk", "xi", "kn", "wm", "g")}
        for form in ("l", "r"):
            with _form(form):
                gfk, _ = hip.fit_many_adjoint_device(dim, order, t["xk"], t["nk"], t["xi"], t["kn"], t["wm"], t["g"], grad_fi=False)
            torch.cuda.synchronize()
            assert torch.equal(_bits(gfk), _bits(got["l"][2])), "%s %s: the fused grad_fk is not the adjoint's (%s)" % (f, shape, form)


# ---- 3. layout edges -------------------------------------------------------------------------------------------------------------------

def _edge_batch(dim, order, K, n):
    """`plain` with ragged nk (0 and K among them, otherwise at least unknowns + 2), every fourth case from 3 on with every DOF known."""
    b = A.op_batch("plain", dim, order, K, n)
    no = b["no"]
    rng = np.random.default_rng(1000 * dim + 10 * order + K)
    nk = rng.integers(min(no + 2, K), K + 1, n).astype(np.int32)
    nk[0], nk[1], nk[n - 1] = K, 0, 0
    b["nk"] = nk
    b["kn"] = b["kn"].copy()
    b["kn"][3::4] = (1 << no) - 1
    b["g"] = A.op_g("plain", dim, order, K, n)
    return b


@pytest.mark.parametrize("dim,order,K,n", [(1, 2, 7, 127), (3, 1, 9, 65), (2, 2, 32, 65)], ids=lambda v: str(v))
def test_layout_edges(hip, dim, order, K, n):
    """Ragged nk with 0 and K, an odd K * dim (the 8-byte tail of the wave's run), a tail group of fewer than 64 cases, cases with every
    DOF known: exact zeros in the padding and for the all-known cases, both forms the same bits, and against the truth and the
    reference under criterion (a) on the cases that have neighbours."""
    import torch
    b = _edge_batch(dim, order, K, n)
    fi = _forward(hip, b)
    got = {}
    for form, kernel in FORMS:
        out = _geometry(hip, b, fi, form, n=n)
        assert out[3] == kernel
        got[form] = out
    for i in range(3):
        assert torch.equal(_bits(got["l"][i]), _bits(got["r"][i]))
    gxk, gxi, gfk = (got["r"][i].cpu().numpy() for i in range(3))
    gxk, gxi = gxk.reshape(n, K, dim), gxi.reshape(n, dim)
    rows = np.arange(K)[None, :] < b["nk"][:, None]
    assert np.all(gxk[~rows] == 0.0) and np.all(gfk[~rows] == 0.0)
    full = b["kn"] == (1 << b["no"]) - 1
    assert full.sum() > 10 and np.all(gxk[full] == 0.0) and np.all(gxi[full] == 0.0) and np.all(gfk[full] == 0.0)
    assert np.all(gxi[b["nk"] == 0] == 0.0)
    live = b["nk"] > 0
    sub = {k: b[k][live] for k in ("xk", "fk", "nk", "xi", "fi0", "kn", "wm", "g")}
    t_xk, t_xi, s, kappa = G.truth_geometry_adjoint_mp(dim, sub["xk"], sub["fk"], sub["nk"], sub["xi"], sub["fi0"], order, sub["kn"],
                                                       sub["wm"], sub["g"])
    ref = G.geometry_adjoint_ref(dim, order, sub["xk"], sub["fk"], sub["nk"], sub["xi"], sub["fi0"], sub["kn"], sub["wm"], sub["g"])
    m = int(live.sum())
    for name, a, r, t in (("grad_xk", _flat(gxk[live], m), _flat(ref["grad_xk"], m), _flat(t_xk, m)), ("grad_xi", gxi[live], ref["grad_xi"], t_xi)):
        e_cr, e_ct, e_rt = P.grad_err(a, r, s), P.grad_err(a, t, s), P.grad_err(r, t, s)
        print("edges %dD o%d K%d n%d %s: err gpu %.3g ref %.3g" % (dim, order, K, n, name, e_ct.max(), e_rt.max()))
        P.assert_scaled(e_cr, e_ct, e_rt, "layout edges " + name)


def test_strided_rows_run_the_lane_form(hip):
    import torch
    b = _shape_data((2, 2, 32))["plain"]
    fi = _forward(hip, b)
    base = _geometry(hip, b, fi, "l")
    for form in (None, "r"):
        out = _geometry(hip, b, fi, form, strided=True)
        assert out[3] == "geometry-adjoint-lane"
        for i in range(3):
            assert torch.equal(_bits(out[i]), _bits(base[i]))


def test_case_index_restricts_the_launch(hip):
    import torch
    b = _shape_data((2, 2, 32))["plain"]
    fi = _forward(hip, b)
    base = _geometry(hip, b, fi, "l")
    sel = np.arange(3, N, 7).astype(np.int64)
    gxk, gxi, gfk = _nan(N, 32, 2), _nan(N, 2), _nan(N, 32)
    hip.fit_many_geometry_adjoint_device(2, 2, _dev(b["xk"]), _dev(b["fk"]), _dev(b["nk"]), _dev(b["xi"]), fi, _dev(b["kn"]), _dev(b["wm"]),
                                         _dev(b["g"]), grad_xk=gxk, grad_xi=gxi, grad_fk=gfk, case_index=_dev(sel))
    assert hip.last_kernel() == "geometry-adjoint-lane"
    torch.cuda.synchronize()
    rest = np.setdiff1d(np.arange(N), sel)
    for got, want in ((gxk, base[0]), (gxi, base[1]), (gfk, base[2])):
        assert torch.isnan(got[rest]).all()
        assert torch.equal(_bits(got[sel]), _bits(want[sel]))


def test_unsupported_shape_is_a_value_error_from_the_library(hip):
    import ctypes as C
    from wlsqm import _binding as B
    t = dict(xk=_nan(8, 40, 3), fk=_nan(8, 40), xi=_nan(8, 3), fi=_nan(8, 20), g=_nan(8, 20), gxk=_nan(8, 40, 3), gxi=_nan(8, 3))
    nk, kn, wm = _dev(np.full(8, 40, np.int32)), _dev(np.zeros(8, np.int64)), _dev(np.full(8, 2, np.int32))
    b = B.Batch()
    b.dimension, b.ncases, b.max_nk = 3, 8, 40
    b.xk, b.xk_stride_case, b.xk_stride_k = t["xk"].data_ptr(), 120, 3
    b.fk, b.fk_stride_case, b.fk_stride_k = t["fk"].data_ptr(), 40, 1
    b.fi, b.fi_stride_case = t["fi"].data_ptr(), 20
    b.nk, b.nk_stride, b.xi, b.xi_stride_case = nk.data_ptr(), 1, t["xi"].data_ptr(), 3
    b.knowns, b.knowns_stride, b.weighting_method, b.wm_stride = kn.data_ptr(), 1, wm.data_ptr(), 1
    call = lambda order: B.lib().wlsqm_hip_fit_geometry_adjoint_device(C.byref(b), 0, None, order, t["g"].data_ptr(), 20, t["gxk"].data_ptr(),
                                                                      120, 3, t["gxi"].data_ptr(), 3, None, 0, 0, None, 0)
    assert call(3) == B.WLSQM_EVALUE
    assert B.lib().wlsqm_hip_last_error().decode() == "fit_geometry_adjoint: unsupported (dimension, order)"
    b.do_sens = 1
    assert call(2) == B.WLSQM_EVALUE


# ---- 4. index-based --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ((2, 2, 32), (3, 2, 40), (1, 2, 8)), ids=_ids)
def test_index_based_form(hip, shape):
    """Point tables built from the family batches (A.point_table) and the real lattice, whose rows start with the node itself: the
    per-slot gradients, the own-point rows and the fused per-slot grad_F are the dense lane form's bits; grad_S is the numpy scatter of
    slots and own rows to 1e-14 of its scale (index_add_'s order is not fixed; a point receives at most N + 1 contributions)."""
    import torch
    dim, order, K = shape
    data = _shape_data(shape)
    for f in ("plain", "self", "grid", "lattice"):
        b = data[f]
        S, F, hoods, pidx = (b["S"], b["F"], b["hoods"], b["pidx"]) if f == "lattice" else A.point_table(b)
        t = dict(S=_dev(S), F=_dev(F), hoods=_dev(hoods), pidx=_dev(pidx), nk=_dev(b["nk"]), kn=_dev(b["kn"]), wm=_dev(b["wm"]), g=_dev(b["g"]))
        fi = _dev(b["fi0"])
        hip.fit_cloud_device(dim, order, t["S"], t["F"], t["hoods"], fi, t["nk"], t["kn"], t["wm"], point_index=t["pidx"], strict=False)
        slots, own, slots_F = _nan(N, K * dim), _nan(N, dim), _nan(N, K)
        grad_S, grad_F = hip.fit_cloud_geometry_adjoint_device(dim, order, t["S"], t["F"], t["hoods"], fi, t["nk"], t["kn"], t["wm"], t["g"],
                                                               point_index=t["pidx"], grad_F=True, slots=slots, own=own, slots_F=slots_F)
        assert hip.last_kernel() == "geometry-adjoint-lane", (f, hip.last_kernel())
        dense = _geometry(hip, b, fi, "l")
        assert torch.equal(_bits(slots), _bits(dense[0].reshape(N, K * dim))), (f, shape)
        assert torch.equal(_bits(own), _bits(dense[1].reshape(N, dim))), (f, shape)
        assert torch.equal(_bits(slots_F), _bits(dense[2])), (f, shape)
        sl, ow, sF = slots.cpu().numpy().reshape(N * K, dim), own.cpu().numpy(), slots_F.cpu().numpy().reshape(-1)
        npts = len(F)
        want, mag = np.zeros((npts, dim)), np.zeros((npts, dim))
        np.add.at(want, hoods.reshape(-1), sl); np.add.at(mag, hoods.reshape(-1), np.abs(sl))
        np.add.at(want, pidx, ow); np.add.at(mag, pidx, np.abs(ow))
        gS = grad_S.cpu().numpy().reshape(npts, dim)
        assert gS.shape == want.shape and tuple(grad_S.shape) == tuple(S.shape)
        assert np.all(np.abs(gS - want) <= 1e-14 * max(mag.max(), np.finfo(np.float64).tiny)), (f, shape, np.abs(gS - want).max(), mag.max())
        wantF = np.zeros(npts)
        np.add.at(wantF, hoods.reshape(-1), sF)
        assert np.all(np.abs(grad_F.cpu().numpy() - wantF) <= 1e-14 * max(np.abs(sF).max(), np.finfo(np.float64).tiny))


def test_ragged_hoods_padding_is_never_dereferenced(hip):
    """Padding of a hoods row set to -1: the kernel never reads it and the scatter points it at point 0 with exact zeros."""
    import torch
    b = _edge_batch(2, 2, 32, 65)
    keep = b["nk"] > 0
    for k in ("xk", "fk", "nk", "xi", "fi0", "kn", "wm", "g"):
        b[k] = b[k][keep]
    n = int(keep.sum())
    b["n"] = n
    S, F, hoods, pidx = A.point_table(b)
    pad = np.arange(32)[None, :] >= b["nk"][:, None]
    hoods_p = hoods.copy(); hoods_p[pad] = -1
    t = dict(S=_dev(S), F=_dev(F), nk=_dev(b["nk"]), kn=_dev(b["kn"]), wm=_dev(b["wm"]), g=_dev(b["g"]), pidx=_dev(pidx))
    fi = _dev(b["fi0"])
    hip.fit_cloud_device(2, 2, t["S"], t["F"], _dev(hoods_p), fi, t["nk"], t["kn"], t["wm"], point_index=t["pidx"], strict=False)
    slots = _nan(n, 64)
    grad_S, _ = hip.fit_cloud_geometry_adjoint_device(2, 2, t["S"], t["F"], _dev(hoods_p), fi, t["nk"], t["kn"], t["wm"], t["g"],
                                                      point_index=t["pidx"], slots=slots)
    torch.cuda.synchronize()
    sl = slots.cpu().numpy().reshape(n, 32, 2)
    assert np.all(sl[pad] == 0.0) and np.isfinite(sl).all()
    gS = grad_S.cpu().numpy()
    # every slot is a point of its own on a point table: the live slots arrive unchanged, the padded ones and point 0's own row aside
    assert _same_bits(gS[n:].reshape(n, 32, 2)[~pad], sl[~pad])
    assert np.all(gS[n:].reshape(n, 32, 2)[pad] == 0.0)


# ---- 5. autograd -------------------------------------------------------------------------------------------------------------------------

def _count_launches(monkeypatch, hip):
    """The list that the four explicit vector-Jacobian products of wlsqm.hip append their names to from now on (the backward pass runs
    on autograd's thread, whose last_kernel() the test's thread does not see): what a backward pass launched, in order."""
    calls = []
    for name in ("fit_many_adjoint_device", "fit_many_geometry_adjoint_device", "fit_cloud_adjoint_device",
                 "fit_cloud_geometry_adjoint_device"):
        def wrap(*a, _real=getattr(hip, name), _name=name, **kw):
            calls.append(_name)
            return _real(*a, **kw)
        monkeypatch.setattr(hip, name, wrap)
    return calls


def test_autograd_reaches_the_coordinates(hip, monkeypatch):
    import torch
    b = _shape_data((2, 2, 32))["plain"]
    t = {k: _dev(b[k]) for k in ("xk", "fk", "nk", "xi", "fi0", "kn", "wm", "g")}
    fi_out = _forward(hip, b)
    with _form(None):
        gxk_x, gxi_x, gfk_x = hip.fit_many_geometry_adjoint_device(2, 2, t["xk"], t["fk"], t["nk"], t["xi"], fi_out, t["kn"], t["wm"], t["g"],
                                                                   grad_fk=True)
        _, gfi_x = hip.fit_many_adjoint_device(2, 2, t["xk"], t["nk"], t["xi"], t["kn"], t["wm"], t["g"])
        calls = _count_launches(monkeypatch, hip)
        # everything that can want a gradient
        xk, xi, fk, fi = (t[k].clone().requires_grad_() for k in ("xk", "xi", "fk", "fi0"))
        out = hip.differentiable_fit_many(2, 2, xk, fk, t["nk"], xi, fi, t["kn"], t["wm"], geometry=True)
        assert torch.equal(_bits(out.detach()), _bits(fi_out)) and torch.equal(_bits(fi.detach()), _bits(t["fi0"]))
        (out * t["g"]).sum().backward()
        assert calls == ["fit_many_geometry_adjoint_device", "fit_many_adjoint_device"]     # fi wants its gradient: the existing adjoint too
        for got, want in ((xk.grad, gxk_x), (xi.grad, gxi_x), (fk.grad, gfk_x), (fi.grad, gfi_x)):
            assert torch.equal(_bits(got), _bits(want))
        # the coordinates and fk: the geometry kernel alone, fk through its fused output
        xk, xi, fk = (t[k].clone().requires_grad_() for k in ("xk", "xi", "fk"))
        out = hip.differentiable_fit_many(2, 2, xk, fk, t["nk"], xi, t["fi0"], t["kn"], t["wm"], geometry=True)
        del calls[:]
        (out * t["g"]).sum().backward()
        assert calls == ["fit_many_geometry_adjoint_device"]            # no launch of the existing adjoint
        for got, want in ((xk.grad, gxk_x), (xi.grad, gxi_x), (fk.grad, gfk_x)):
            assert torch.equal(_bits(got), _bits(want))
        # xi alone
        xi = t["xi"].clone().requires_grad_()
        out = hip.differentiable_fit_many(2, 2, t["xk"], t["fk"], t["nk"], xi, t["fi0"], t["kn"], t["wm"], geometry=True)
        del calls[:]
        (out * t["g"]).sum().backward()
        assert calls == ["fit_many_geometry_adjoint_device"] and torch.equal(_bits(xi.grad), _bits(gxi_x))
        # fk alone: the existing adjoint, no geometry kernel
        fk = t["fk"].clone().requires_grad_()
        out = hip.differentiable_fit_many(2, 2, t["xk"], fk, t["nk"], t["xi"], t["fi0"], t["kn"], t["wm"], geometry=True)
        del calls[:]
        (out * t["g"]).sum().backward()
        assert calls == ["fit_many_adjoint_device"] and torch.equal(_bits(fk.grad), _bits(gfk_x))
        # nothing requires a gradient: nothing to differentiate, nothing launched
        del calls[:]
        out = hip.differentiable_fit_many(2, 2, t["xk"], t["fk"], t["nk"], t["xi"], t["fi0"], t["kn"], t["wm"], geometry=True)
        assert not out.requires_grad and calls == []
    # the default still refuses
    with pytest.raises(ValueError, match="geometry is not differentiable"):
        hip.differentiable_fit_many(2, 2, t["xk"].clone().requires_grad_(), t["fk"], t["nk"], t["xi"], t["fi0"], t["kn"], t["wm"])


def test_autograd_reaches_the_point_table(hip, monkeypatch):
    import torch
    b = _shape_data((2, 2, 32))["lattice"]
    t = dict(S=_dev(b["S"]), F=_dev(b["F"]), hoods=_dev(b["hoods"]), pidx=_dev(b["pidx"]), nk=_dev(b["nk"]), kn=_dev(b["kn"]),
             wm=_dev(b["wm"]), g=_dev(b["g"]), fi0=_dev(b["fi0"]))
    fi_out = t["fi0"].clone()
    hip.fit_cloud_device(2, 2, t["S"], t["F"], t["hoods"], fi_out, t["nk"], t["kn"], t["wm"], point_index=t["pidx"])
    slots, own, slots_F = _nan(N, 64), _nan(N, 2), _nan(N, 32)
    hip.fit_cloud_geometry_adjoint_device(2, 2, t["S"], t["F"], t["hoods"], fi_out, t["nk"], t["kn"], t["wm"], t["g"], point_index=t["pidx"],
                                          grad_F=True, slots=slots, own=own, slots_F=slots_F)
    S, F = t["S"].clone().requires_grad_(), t["F"].clone().requires_grad_()
    out = hip.differentiable_fit_cloud(2, 2, S, F, t["hoods"], t["fi0"], t["nk"], t["kn"], t["wm"], point_index=t["pidx"], geometry=True)
    assert torch.equal(_bits(out.detach()), _bits(fi_out))
    calls = _count_launches(monkeypatch, hip)
    (out * t["g"]).sum().backward()
    assert calls == ["fit_cloud_geometry_adjoint_device"]              # F through the fused output: no launch of the existing adjoint
    torch.cuda.synchronize()
    # S.grad against the float64 numpy scatter of the explicit call's slots and own rows
    sl, ow = slots.cpu().numpy().reshape(N * 32, 2), own.cpu().numpy()
    want, mag = np.zeros(b["S"].shape), np.zeros(b["S"].shape)
    np.add.at(want, b["hoods"].reshape(-1), sl); np.add.at(mag, b["hoods"].reshape(-1), np.abs(sl))
    np.add.at(want, b["pidx"], ow); np.add.at(mag, b["pidx"], np.abs(ow))
    assert np.abs(want).max() > 0
    assert np.all(np.abs(S.grad.cpu().numpy() - want) <= 1e-14 * mag.max())
    wantF = np.zeros(len(b["F"]))
    np.add.at(wantF, b["hoods"].reshape(-1), slots_F.cpu().numpy().reshape(-1))
    assert np.all(np.abs(F.grad.cpu().numpy() - wantF) <= 1e-14 * np.abs(wantF).max())
    with pytest.raises(ValueError, match="geometry is not differentiable"):
        hip.differentiable_fit_cloud(2, 2, t["S"].clone().requires_grad_(), t["F"], t["hoods"], t["fi0"], t["nk"], t["kn"], t["wm"],
                                     point_index=t["pidx"])


# ---- 6. capture --------------------------------------------------------------------------------------------------------------------------

def test_the_explicit_call_replays_from_a_graph(hip):
    """The forward fit and the geometry adjoint recorded as one chain on one stream (a single branch: two kernels in a row); replayed with
    new g: the eager results' bits."""
    import torch
    b = _shape_data((2, 2, 32))["plain"]
    t = {k: _dev(b[k]) for k in ("xk", "fk", "nk", "xi", "fi0", "kn", "wm")}
    fi, g = t["fi0"].clone(), _dev(b["g"])
    gxk, gxi, gfk = _nan(N, 32, 2), _nan(N, 2), _nan(N, 32)

    def step():
        fi.copy_(t["fi0"])
        hip.fit_many_device(2, 2, t["xk"], t["fk"], t["nk"], t["xi"], fi, t["kn"], t["wm"])
        hip.fit_many_geometry_adjoint_device(2, 2, t["xk"], t["fk"], t["nk"], t["xi"], fi, t["kn"], t["wm"], g, grad_xk=gxk, grad_xi=gxi,
                                             grad_fk=gfk)

    step()                                                            # warm-up outside the capture
    torch.cuda.synchronize()
    gxk.fill_(-7.0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        step()
    torch.cuda.synchronize()
    assert float(gxk.min()) == -7.0 and float(gxk.max()) == -7.0      # captured, not run
    for seed in (1, 2):
        g.copy_(_dev(np.random.default_rng(seed).uniform(-1, 1, (N, 6))))
        graph.replay()
        torch.cuda.synchronize()
        got = (gxk.clone(), gxi.clone(), gfk.clone())
        gxk.fill_(-7.0); gxi.fill_(-7.0); gfk.fill_(-7.0)
        step()
        torch.cuda.synchronize()
        for a, c in zip(got, (gxk, gxi, gfk)):
            assert torch.equal(_bits(a), _bits(c))
