"""CPU-only checks around the fit's geometry adjoint (wlsqm.hip.fit_many_geometry_adjoint_device and friends):
the mpmath truth of tests/_geometry_adjoint_ref.py pinned to central differences, the fp64 numpy reference rehearsed on every family the
GPU tests use, the condition under which the farthest neighbour of the kernels is the exact one, and the host-side surface."""
import os
import re

import numpy as np
import pytest

import _adversarial as A
import _cases as K
import _geometry_adjoint_ref as G
import _parity as P
from _device_helpers import OnDevice as _OnDevice

ROOT = K.ROOT
WORKERS = max(1, min(12, os.cpu_count() or 1))

PIN_SHAPES = ((1, 2, 8), (1, 4, 12), (2, 2, 12), (2, 3, 16), (3, 2, 14))


@pytest.mark.parametrize("dim,order,Kn", PIN_SHAPES, ids=lambda v: str(v))
def test_truth_equals_central_differences(dim, order, Kn):
    """truth_geometry_adjoint_mp against mpmath central differences of g . fi_out at 80 digits, step 1e-25 of the neighbourhood size: both
    weightings, three masks (none, F known, a stray high bit), 3 cases each, the truth taken before its one rounding (as_mp=True).
    Bar: 1e-30 of the case's scale s.  The step's truncation error is of the order of (1e-25)^2 = 1e-50 of the gradient, the rounding
    of the quotient 1e-80 / 1e-25 = 1e-55 times the conditioning: 20 orders of margin, and far below anything fp64 can see.
    fit_value_mp, the function that is differenced (a double cannot hold such a step, so truth_fit_mp cannot be differenced itself),
    is first held to truth_fit_mp at the unperturbed point."""
    from mpmath import mp, mpf
    n = 3
    no = A.NDOF[dim][order]
    b = A.make("plain", dim, order, Kn, n)
    g = A.op_g("plain", dim, order, Kn, n)
    worst = 0.0
    for wmv in (2, 1):
        for mask in (0, 1, 1 << (no + 1)):
            kn, wm = np.full(n, mask, np.int64), np.full(n, wmv, np.int32)
            gxk, gxi, s, kappa = G.truth_geometry_adjoint_mp(dim, b["xk"], b["fk"], b["nk"], b["xi"], b["fi0"], order, kn, wm, g, as_mp=True)
            assert np.isfinite(gxk.astype(float)).all() and np.abs(gxk.astype(float)).max() > 0
            with mp.workdps(80):
                full, _ = P.truth_fit_mp(dim, b["xk"], b["fk"], b["nk"], b["xi"], b["fi0"], b["order_a"], kn, wm, dps=80, as_mp=True)
                for j in range(n):
                    xk = b["xk"][j].reshape(Kn, dim)
                    xi = np.asarray(b["xi"][j]).reshape(dim)
                    d0 = [[mpf(float(xk[k, m])) - mpf(float(xi[m])) for m in range(dim)] for k in range(Kn)]
                    value = lambda d: G.fit_value_mp(dim, order, d, b["fk"][j], b["fi0"][j], mask, wmv == 1, g[j])
                    L0 = mp.fsum(mpf(float(g[j, a])) * full[j, a] for a in range(no))
                    assert abs(value(d0) - L0) <= mpf(10) ** -50 * max(abs(L0), 1)
                    h = mpf(10) ** -25 * mpf(A.H)
                    tot = [mpf(0)] * dim
                    for k in range(Kn):
                        for m in range(dim):
                            up = [list(r) for r in d0]; dn = [list(r) for r in d0]
                            up[k][m] += h; dn[k][m] -= h
                            fd = (value(up) - value(dn)) / (2 * h)
                            tot[m] -= fd
                            assert abs(fd - gxk[j, k, m]) <= mpf(10) ** -30 * mpf(float(s[j])), (dim, order, wmv, mask, j, k, m)
                    for m in range(dim):
                        assert abs(tot[m] - gxi[j, m]) <= mpf(10) ** -30 * mpf(float(s[j])), (dim, order, wmv, mask, j, m)
            worst = max(worst, float(np.abs(gxk.astype(float)).max()))
    assert worst > 0


@pytest.fixture(scope="module")
def truths():
    """shape -> family -> (grad_xk, grad_xi, s, kappa), computed once in worker processes; nothing below modifies it."""
    return {shape: G.geometry_truths(shape, G.FAMILIES, workers=WORKERS) for shape in G.SHAPES}


@pytest.mark.parametrize("shape", G.SHAPES, ids=lambda s: "%dD-o%d-K%d" % s)
def test_reference_rehearsed_on_every_family(truths, shape):
    """geometry_adjoint_ref on every family but the two *_edge ones, 96 cases each: finite, and its q against the truth printed (the
    figure the GPU's is compared with)."""
    dim, order, Kn = shape
    for f in G.FAMILIES:
        b = A.op_batch(f, dim, order, Kn)
        g = A.op_g(f, dim, order, Kn)
        ref = G.geometry_adjoint_ref(dim, order, b["xk"], b["fk"], b["nk"], b["xi"], b["fi0"], b["kn"], b["wm"], g)
        t_xk, t_xi, s, kappa = truths[shape][f]
        assert np.isfinite(ref["grad_xk"]).all() and np.isfinite(ref["grad_xi"]).all(), (f, shape)
        assert np.isfinite(t_xk).all() and np.isfinite(t_xi).all() and np.isfinite(kappa).all(), (f, shape)
        q_xk = P.grad_q(ref["grad_xk"].reshape(A.N_OP, -1), t_xk.reshape(A.N_OP, -1), s, kappa)
        q_xi = P.grad_q(ref["grad_xi"], t_xi, s, kappa)
        print("%-12s %dD order %d K %2d  kappa %.3g  max q of the reference: grad_xk %.3g  grad_xi %.3g"
              % (f, dim, order, Kn, kappa.max(), q_xk.max(), q_xi.max()))


@pytest.mark.parametrize("shape", G.SHAPES, ids=lambda s: "%dD-o%d-K%d" % s)
def test_farthest_neighbour_in_fp64_is_the_exact_one(shape):
    """What keeps the per-case criterion honest: the kernels and the reference take k* from fp64 squared distances, the truth from exact
    ones.  On every case of every family (the *_edge ones included; no case is excluded) the first index of the largest fp64 d2 is the
    smallest index of the largest exact d2.  Exact ties occur on the lattice families and exercise the smaller-index rule."""
    dim, order, Kn = shape
    ties = 0
    for f in A.OP_FAMILIES:
        b = A.op_batch(f, dim, order, Kn)
        kk = G.farthest_first(dim, b["xk"], b["nk"], b["xi"])
        assert len(kk) == A.N_OP
        differ = int((kk[:, 0] != kk[:, 1]).sum())
        assert differ == 0, "%s %s: %d of %d cases pick another farthest neighbour in fp64" % (f, shape, differ, A.N_OP)
        if f in ("grid", "grid_sorted", "lattice"):
            x = b["xk"].reshape(A.N_OP, Kn, -1) - np.asarray(b["xi"]).reshape(A.N_OP, 1, -1)
            d2 = (x * x).sum(axis=-1)
            ties += int(((d2 == d2.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
    assert ties > 0 or dim == 1


# ---- the host-side surface ----

def _args(n=4, K_=7, dim=2, no=6):
    import torch
    gen = torch.Generator().manual_seed(0)
    return dict(xk=torch.rand((n, K_, dim), dtype=torch.float64, generator=gen), fk=torch.rand((n, K_), dtype=torch.float64, generator=gen),
                nk=torch.full((n,), K_, dtype=torch.int32), xi=torch.zeros((n, dim), dtype=torch.float64),
                fi_out=torch.zeros((n, no), dtype=torch.float64), knowns=torch.zeros((n,), dtype=torch.int64),
                weighting_method=torch.full((n,), 2, dtype=torch.int32), g=torch.ones((n, no), dtype=torch.float64))


def test_the_names_exist():
    import wlsqm
    import wlsqm.hip as h
    for name in ("fit_many_geometry_adjoint_device", "fit_cloud_geometry_adjoint_device"):
        assert callable(getattr(h, name)) and name in h.__all__
        assert not hasattr(wlsqm, name)


def test_argument_errors_are_raised_before_the_library_is_reached():
    import wlsqm.hip as h
    t = _args()
    f = h.fit_many_geometry_adjoint_device
    with pytest.raises(ValueError, match="must be a device"):
        f(2, 2, **t)
    dev = {k: _OnDevice(v) for k, v in t.items()}
    with pytest.raises(ValueError, match="dtype mismatch"):
        f(2, 2, **dict(dev, nk=_OnDevice(t["nk"].long())))
    with pytest.raises(ValueError, match="dtype mismatch"):
        f(2, 2, **dict(dev, fk=_OnDevice(t["fk"].float())))
    with pytest.raises(ValueError, match="dtype mismatch"):
        f(2, 2, **dict(dev, fi_out=_OnDevice(t["fi_out"].float())))
    with pytest.raises(ValueError, match="wrong number of dimensions"):
        f(2, 2, **dict(dev, xk=_OnDevice(t["xk"][:, :, 0])))
    with pytest.raises(ValueError, match="not contiguous in the same dimension"):
        f(2, 2, **dict(dev, g=_OnDevice(t["g"].repeat(1, 2)[:, ::2])))
    with pytest.raises(ValueError, match="columns"):
        f(2, 2, **dict(dev, fi_out=_OnDevice(t["fi_out"][:, :5])))
    with pytest.raises(ValueError, match="rows"):
        f(2, 2, **dict(dev, g=_OnDevice(t["g"][:3])))
    with pytest.raises(ValueError, match="neighbour slots"):
        f(2, 2, **dict(dev, fk=_OnDevice(t["fk"].repeat(1, 2))))
    with pytest.raises(ValueError, match="grad_xk"):
        f(2, 2, grad_xk=_OnDevice(t["xk"][:, :5]), **dev)
    with pytest.raises(ValueError, match="grad_xi"):
        f(2, 2, grad_xk=_OnDevice(t["xk"].clone()), grad_xi=_OnDevice(t["xi"][:3]), **dev)
    with pytest.raises(ValueError, match="order must be"):
        f(2, 5, **dev)
    t3 = _args(dim=3, no=20)
    with pytest.raises(ValueError, match=r"unsupported \(dimension, order\)"):
        f(3, 3, **{k: _OnDevice(v) for k, v in t3.items()})
    with pytest.raises(ValueError, match="integer order"):
        f(2, _OnDevice(t["nk"]), **dev)
    import torch
    S = torch.rand((9, 2), dtype=torch.float64)
    c = dict(S=S, F=torch.rand((9,), dtype=torch.float64), hoods=torch.zeros((4, 7), dtype=torch.int32), nk=t["nk"], fi_out=t["fi_out"],
             knowns=t["knowns"], weighting_method=t["weighting_method"], g=t["g"])
    fc = h.fit_cloud_geometry_adjoint_device
    with pytest.raises(ValueError, match="must be a device"):
        fc(2, 2, **c)
    cd = {k: _OnDevice(v) for k, v in c.items()}
    with pytest.raises(ValueError, match="dtype mismatch"):
        fc(2, 2, **dict(cd, hoods=_OnDevice(c["hoods"].long())))
    with pytest.raises(ValueError, match="fewer entries"):
        fc(2, 2, **dict(cd, F=_OnDevice(c["F"][:5])))
    with pytest.raises(ValueError, match="grad_S"):
        fc(2, 2, grad_S=_OnDevice(S[:5]), slots=_OnDevice(torch.zeros((4, 14), dtype=torch.float64)),
           own=_OnDevice(torch.zeros((4, 2), dtype=torch.float64)), **cd)
    with pytest.raises(ValueError, match="slots must be at least"):
        fc(2, 2, slots=_OnDevice(torch.zeros((4, 7), dtype=torch.float64)), **cd)


def test_geometry_false_still_refuses_the_gradient():
    import wlsqm.hip as h
    t = _args()
    for kw in ({}, {"geometry": False}):
        with pytest.raises(ValueError, match="geometry is not differentiable"):
            h.differentiable_fit_many(2, 2, t["xk"].clone().requires_grad_(), t["fk"], t["nk"], t["xi"], t["fi_out"], t["knowns"],
                                      t["weighting_method"], **kw)
        with pytest.raises(ValueError, match="geometry is not differentiable"):
            h.differentiable_fit_cloud(2, 2, t["xk"][:, 0].clone().requires_grad_(), t["fk"][:, 0], t["nk"].reshape(4, 1), t["fi_out"],
                                       t["nk"], t["knowns"], t["weighting_method"], **kw)


def test_both_symbols_are_declared_in_the_header():
    hdr = open(os.path.join(ROOT, "include", "wlsqm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("wlsqm_hip_fit_geometry_adjoint_device", "wlsqm_hip_fit_cloud_geometry_adjoint_device"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
