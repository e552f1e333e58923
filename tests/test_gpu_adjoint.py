"""GPU tests of the fit's adjoint (csrc/fit_adjoint.hip; wlsqm.hip.fit_many_adjoint_device, fit_cloud_adjoint_device and the two
autograd wrappers).  Criterion everywhere: per case e_j = ||cand_j - ref_j||_inf / s[j] <= TOL + NOISE_MULT * N, with the project's
TOL and NOISE_MULT (tests/_parity.py), s[j] the case's scale and N the fp64 noise floor of the quantity, both from
tests/_adjoint_ref.py: N is recomputed here from the golden sweeps (the oracle's sensitivities against the real reference's).
Only cases with fewer neighbours than unknowns + 2 are left out of a maximum, and their share is asserted."""
import os

import numpy as np
import pytest

import _adjoint_ref as R
import _cases as K
import _parity as P
from _device_helpers import bits as _bits, dev as _dev, nan as _nan

pytestmark = pytest.mark.gpu

SWITCH = "WLSQM_HIP_ADJOINT_FORM"


@pytest.fixture(scope="module")
def hip():
    import wlsqm.hip as h
    from wlsqm import _binding
    assert _binding.lib().wlsqm_hip_device_count() >= 1, "no HIP device: the GPU tests need a real MI355X"
    return h


@pytest.fixture(scope="module")
def floors():
    """dim -> (N, pieces) of the reference sweeps, computed once and shared; nothing below modifies it."""
    return {dim: R.noise_floor(dim) for dim in (1, 2, 3)}


def _bar(floors, dim):
    return P.TOL + P.NOISE_MULT * floors[dim][0]


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


def _err(cand, ref, s):
    with np.errstate(invalid="ignore"):
        e = np.abs(cand - ref).max(axis=1) / s
    return np.where(np.isfinite(e), e, np.inf)


# ---- 1. the reference sweeps ----

@pytest.mark.parametrize("dim", [1, 2, 3])
def test_reference_sweeps(hip, floors, dim):
    """Every order 0-4 (3D: 0-2), masks including the stray-high-bit ones, both weightings, ragged nk: grad_fk against the contraction
    of the real reference's golden sensitivities, grad_fi against the oracle's exact-linearity construction; bucketed by order with
    case_index as the forward sweep tests are."""
    import torch
    N, x = floors[dim]
    d, g, ref = x["d"], x["g"], x["ref"]
    n, Kn = d["fk"].shape
    no_max = g.shape[1]
    t = {k: _dev(d[k]) for k in ("xk", "nk", "xi", "knowns", "wm")}
    g_d = _dev(g)
    gfk, gfi = _nan(n, Kn), _nan(n, no_max)
    for o in range(5):
        if not R.covered(dim, o):
            continue
        idx = torch.from_numpy(np.where(d["order"] == o)[0].astype(np.int64)).cuda()
        hip.fit_many_adjoint_device(dim, o, t["xk"], t["nk"], t["xi"], t["knowns"], t["wm"], g_d, grad_fk=gfk, grad_fi=gfi, case_index=idx)
        assert hip.last_kernel() == "adjoint-lane"                    # case_index: the lane form
    torch.cuda.synchronize()
    gfk, gfi = gfk.cpu().numpy(), gfi.cpu().numpy()
    use = x["use"]
    cov = x["cov"]
    assert (~x["ok"][cov]).mean() <= (~x["suite"][cov]).mean()        # left out: no more than the existing suites' rule (nk < no + 2) skips here
    assert np.all(np.isnan(gfk[~x["cov"]])) and np.all(np.isnan(gfi[~x["cov"]]))     # rows no bucket named keep their pre-fill
    bar = _bar(floors, dim)
    e_fk = _err(gfk, x["gold_fk"], ref["s"])
    e_fi = np.zeros(n)
    for j in np.where(use)[0]:
        no = K.NDOF[dim][int(d["order"][j])]
        e_fi[j] = np.abs(gfi[j, :no] - ref["grad_fi"][j, :no]).max() / ref["s"][j]
        assert np.all(np.isnan(gfi[j, no:]))                          # columns beyond `no` untouched
    print("sweep_%dd: N = %.3e, bar = %.3e, grad_fk max e = %.3e, grad_fi max e = %.3e over %d cases"
          % (dim, N, bar, e_fk[use].max(), e_fi[use].max(), int(use.sum())))
    assert e_fk[use].max() <= bar, (int(np.argmax(np.where(use, e_fk, 0))), e_fk[use].max())
    assert e_fi[use].max() <= bar
    live = np.arange(Kn)[None, :] < d["nk"][:, None]
    assert np.all(gfk[x["cov"]][~live[x["cov"]]] == 0.0)               # padding: exact zeros


# ---- 2. both forms on the smallest shapes that can go wrong ----

def _synthetic(dim, order, Kn, n, mask, seed):
    """A synthetic cloud problem with ragged neighbour counts (at least three quarters of the row, and never fewer than unknowns + 2)."""
    import synth
    rng = np.random.default_rng(seed)
    no = K.NDOF[dim][order]
    if dim == 1:
        S = np.sort(rng.uniform(0.0, 1.0, max(4 * n, 64)))
        hoods = synth.knn(S[:, None], Kn, query=np.arange(n))
        xk, xi = S[hoods], S[:n].copy()
    else:
        p = synth.cloud_problem(dim, max(4 * n, 4 * Kn), Kn, ncases=n)
        xk, xi = p["xk"], p["xi"]
    if mask == "random":
        knowns = rng.integers(0, 1 << no, n).astype(np.int64)
    elif mask == "some_full":
        knowns = np.where(rng.uniform(size=n) < 0.25, (1 << no) - 1, 0).astype(np.int64)
        knowns[0] = (1 << no) - 1
    else:
        knowns = np.full(n, int(mask), np.int64)
    lo = max(no + 2, (3 * Kn) // 4)
    nk = rng.integers(min(lo, Kn), Kn + 1, n).astype(np.int32)
    nk[0] = Kn
    wm = np.where(rng.uniform(size=n) < 0.2, 1, 2).astype(np.int32)
    g = rng.uniform(-1.0, 1.0, (n, no))
    ref = R.adjoint_ref(dim, order, xk, nk, xi, knowns, wm, g)
    ok, _ = R.resolvable(dim, np.full(n, order), nk, knowns)
    assert ok.all()                                                   # nothing is left out of the maximum on the synthetic clouds
    return dict(dim=dim, order=order, K=Kn, n=n, no=no, xk=xk, xi=xi, nk=nk, knowns=knowns, wm=wm, g=g, ref=ref)


SHAPES = [
    # id, dim, order, K, n, mask, the two forms bit for bit
    ("c2-none", 2, 2, 32, 200, 0, True),
    ("c2-F", 2, 2, 32, 200, 1, True),                                # wlsqm.b2_F
    ("c2-random", 2, 2, 32, 200, "random", True),
    ("c2-some-full", 2, 2, 32, 200, "some_full", True),
    ("c5", 3, 2, 40, 130, 0, True),
    ("c3-F", 2, 4, 64, 70, 1, False),
    ("c1-odd", 1, 2, 7, 201, 0, True),                               # odd K * dim, odd count: the 8-aligned tail of the run
    ("one", 2, 2, 32, 1, 0, True),
    ("full-group", 2, 2, 32, 64, 0, True),
]


def _run(hip, c, form, strided=False):
    import torch
    t = {k: _dev(c[k]) for k in ("nk", "xi", "knowns", "wm", "g")}
    if strided:
        wide = torch.zeros((c["n"], 2 * c["K"]) + c["xk"].shape[2:], dtype=torch.float64, device="cuda")
        wide[:, ::2] = _dev(c["xk"])
        xk = wide[:, ::2]
    else:
        xk = _dev(c["xk"])
    gfk, gfi = _nan(c["n"], c["K"]), _nan(c["n"], c["no"])
    with _form(form):
        hip.fit_many_adjoint_device(c["dim"], c["order"], xk, t["nk"], t["xi"], t["knowns"], t["wm"], t["g"], grad_fk=gfk, grad_fi=gfi)
        kernel = hip.last_kernel()
    torch.cuda.synchronize()
    return gfk, gfi, kernel


@pytest.mark.parametrize("name,dim,order,Kn,n,mask,bitwise", SHAPES, ids=[s[0] for s in SHAPES])
def test_both_forms(hip, floors, name, dim, order, Kn, n, mask, bitwise):
    c = _synthetic(dim, order, Kn, n, mask, seed=100 + len(name))
    ref = c["ref"]
    bar = _bar(floors, dim)
    got = {}
    for form, kernel in (("l", "adjoint-lane"), ("r", "adjoint-rows")):
        gfk_d, gfi_d, ran = _run(hip, c, form)
        assert ran == kernel, (form, ran)                             # dense rows within the LDS budget: eligible for either
        gfk, gfi = gfk_d.cpu().numpy(), gfi_d.cpu().numpy()
        got[form] = (gfk_d, gfi_d)
        e_fk, e_fi = _err(gfk, ref["grad_fk"], ref["s"]), _err(gfi, ref["grad_fi"], ref["s"])
        print("%s form %s: bar %.3e, grad_fk max e %.3e, grad_fi max e %.3e" % (name, form, bar, e_fk.max(), e_fi.max()))
        assert e_fk.max() <= bar and e_fi.max() <= bar
        live = np.arange(Kn)[None, :] < c["nk"][:, None]
        assert not np.isnan(gfk).any() and np.all(gfk[~live] == 0.0)  # every slot written; the padding holds exact zeros
        for j in range(n):
            kn = int(c["knowns"][j]) & ((1 << c["no"]) - 1)
            for a in range(c["no"]):
                if not (kn >> a) & 1:
                    assert gfi[j, a] == 0.0                            # unknown: its incoming value is never read
            if kn == (1 << c["no"]) - 1:
                assert np.all(gfk[j] == 0.0) and np.array_equal(gfi[j], c["g"][j])      # the fit's no-op
    import torch
    if bitwise:
        assert torch.equal(_bits(got["l"][0]), _bits(got["r"][0])) and torch.equal(_bits(got["l"][1]), _bits(got["r"][1]))
    else:
        a, b = got["l"][0].cpu().numpy(), got["r"][0].cpu().numpy()
        assert _err(a, b, ref["s"]).max() <= bar
        assert _err(got["l"][1].cpu().numpy(), got["r"][1].cpu().numpy(), ref["s"]).max() <= bar


def test_dropped_columns_pass_g_through(hip, floors):
    """Stray high mask bits drop the last unknowns: grad_fi is exactly g there, in either form."""
    c = _synthetic(2, 2, 32, 70, 0, seed=5)
    c["knowns"] = np.full(c["n"], (1 << 9) | 2, np.int64)             # DOF 1 known, one stray bit: DOF 5 dropped
    c["ref"] = R.adjoint_ref(2, 2, c["xk"], c["nk"], c["xi"], c["knowns"], c["wm"], c["g"])
    for form in ("l", "r"):
        gfk, gfi, _ = _run(hip, c, form)
        gfk, gfi = gfk.cpu().numpy(), gfi.cpu().numpy()
        assert np.array_equal(gfi[:, 5], c["g"][:, 5])
        assert np.all(gfi[:, [0, 2, 3, 4]] == 0.0)
        assert _err(gfk, c["ref"]["grad_fk"], c["ref"]["s"]).max() <= _bar(floors, 2)
        assert _err(gfi, c["ref"]["grad_fi"], c["ref"]["s"]).max() <= _bar(floors, 2)


# ---- 3. fallbacks ----

def test_strided_rows_run_the_lane_form(hip):
    import torch
    c = _synthetic(2, 2, 32, 200, 1, seed=9)
    gfk0, gfi0, _ = _run(hip, c, "l")
    for form in (None, "r"):
        gfk, gfi, ran = _run(hip, c, form, strided=True)
        assert ran == "adjoint-lane"
        assert torch.equal(_bits(gfk), _bits(gfk0)) and torch.equal(_bits(gfi), _bits(gfi0))


def test_case_index_restricts_the_launch(hip):
    import torch
    c = _synthetic(2, 2, 32, 200, 0, seed=10)
    gfk0, gfi0, _ = _run(hip, c, "l")
    t = {k: _dev(c[k]) for k in ("xk", "nk", "xi", "knowns", "wm", "g")}
    sel = np.arange(3, 200, 7).astype(np.int64)
    gfk, gfi = _nan(200, 32), _nan(200, 6)
    hip.fit_many_adjoint_device(2, 2, t["xk"], t["nk"], t["xi"], t["knowns"], t["wm"], t["g"], grad_fk=gfk, grad_fi=gfi,
                                case_index=_dev(sel))
    assert hip.last_kernel() == "adjoint-lane"
    torch.cuda.synchronize()
    rest = np.setdiff1d(np.arange(200), sel)
    assert torch.isnan(gfk[rest]).all() and torch.isnan(gfi[rest]).all()
    assert torch.equal(_bits(gfk[sel]), _bits(gfk0[sel])) and torch.equal(_bits(gfi[sel]), _bits(gfi0[sel]))


def test_unsupported_shape_is_a_value_error_from_the_library(hip):
    import ctypes as C
    from wlsqm import _binding as B
    c = _synthetic(3, 2, 40, 8, 0, seed=3)
    t = {k: _dev(c[k]) for k in ("xk", "nk", "xi", "knowns", "wm")}
    g, gfk = _nan(8, 20), _nan(8, 40)
    b = B.Batch()
    b.dimension, b.ncases, b.max_nk = 3, 8, 40
    b.xk, b.xk_stride_case, b.xk_stride_k = t["xk"].data_ptr(), 120, 3
    b.nk, b.nk_stride, b.xi, b.xi_stride_case = t["nk"].data_ptr(), 1, t["xi"].data_ptr(), 3
    b.knowns, b.knowns_stride, b.weighting_method, b.wm_stride = t["knowns"].data_ptr(), 1, t["wm"].data_ptr(), 1
    rc = B.lib().wlsqm_hip_fit_adjoint_device(C.byref(b), 0, None, 3, g.data_ptr(), 20, gfk.data_ptr(), 40, 1, None, 0, None, 0)
    assert rc == B.WLSQM_EVALUE
    assert B.lib().wlsqm_hip_last_error().decode() == "fit_adjoint: unsupported (dimension, order)"
    b.iterative = 1
    assert B.lib().wlsqm_hip_fit_adjoint_device(C.byref(b), 0, None, 2, g.data_ptr(), 20, gfk.data_ptr(), 40, 1, None, 0, None, 0) == B.WLSQM_EVALUE


# ---- 4. autograd ----

def test_autograd_through_fit_many(hip, floors):
    import torch
    c = _synthetic(2, 2, 32, 200, 1, seed=21)
    rng = np.random.default_rng(22)
    t = {k: _dev(c[k]) for k in ("xk", "nk", "xi", "knowns", "wm")}
    fk0, fi0 = _dev(rng.uniform(-1, 1, (200, 32))), _dev(rng.uniform(-1, 1, (200, 6)))
    G = _dev(c["g"])
    gfk_x, gfi_x = hip.fit_many_adjoint_device(2, 2, t["xk"], t["nk"], t["xi"], t["knowns"], t["wm"], G)

    def fit(fk, fi, **kw):
        out = fi.clone()
        hip.fit_many_device(2, 2, t["xk"], fk, t["nk"], t["xi"], out, t["knowns"], t["wm"], **kw)
        return out

    base = fit(fk0, fi0)
    for strict in (None, "accurate"):
        fk, fi = fk0.clone().requires_grad_(), fi0.clone().requires_grad_()
        out = hip.differentiable_fit_many(2, 2, t["xk"], fk, t["nk"], t["xi"], fi, t["knowns"], t["wm"], strict=strict)
        assert torch.equal(_bits(out.detach()), _bits(fit(fk0, fi0, strict=strict)))      # the forward is fit_many_device's bits
        assert torch.equal(_bits(fi.detach()), _bits(fi0))                                  # fi itself is not written
        (out * G).sum().backward()
        # the adjoint does not depend on the forward's numerics mode: the explicit call's bits either way
        assert torch.equal(_bits(fk.grad), _bits(gfk_x)) and torch.equal(_bits(fi.grad), _bits(gfi_x))
    # only the gradient that is needed
    fk = fk0.clone().requires_grad_()
    out = hip.differentiable_fit_many(2, 2, t["xk"], fk, t["nk"], t["xi"], fi0, t["knowns"], t["wm"])
    (out * G).sum().backward()
    assert torch.equal(_bits(fk.grad), _bits(gfk_x))
    # dot-product test against the existing forward
    v, u = _dev(rng.uniform(-1, 1, (200, 32))), _dev(rng.uniform(-1, 1, (200, 6)))
    lhs_terms = (fit(fk0 + v, fi0 + u) - base) * G
    rhs_terms = torch.cat([(v * gfk_x).reshape(-1), (u * gfi_x).reshape(-1)])
    lhs, rhs = float(lhs_terms.sum()), float(rhs_terms.sum())
    scale = float(lhs_terms.abs().sum() + rhs_terms.abs().sum())
    print("dot-product test: lhs %.15e rhs %.15e, |lhs - rhs| / sum|terms| = %.3e" % (lhs, rhs, abs(lhs - rhs) / scale))
    assert abs(lhs - rhs) <= 2.0 * _bar(floors, 2) * scale
    with pytest.raises(ValueError, match="geometry is not differentiable"):
        hip.differentiable_fit_many(2, 2, t["xk"].clone().requires_grad_(), fk0, t["nk"], t["xi"], fi0, t["knowns"], t["wm"])


# ---- 5. index-based ----

@pytest.mark.parametrize("query", ["knn", "ball"])
def test_autograd_through_fit_cloud(hip, query):
    import torch
    import synth
    npts = 300
    S = synth.halton(npts, 2)
    S_d = _dev(S)
    if query == "knn":
        hoods = hip.knn(S_d, 24)
        nk = torch.full((npts,), 24, dtype=torch.int32, device="cuda")
    else:
        hoods, nk = hip.ball(S_d, 0.2, 48)
        hoods = hoods.clone()
        pad = torch.arange(48, device="cuda")[None, :] >= nk[:, None]
        hoods[pad] = -1                                               # the padding of a ragged row is never dereferenced
        assert 6 <= int(nk.min()) < int(nk.max())                     # ragged, padded rows; enough neighbours for 6 unknowns
    Kn = int(hoods.shape[1])
    knowns = torch.zeros((npts,), dtype=torch.int64, device="cuda")
    wm = torch.full((npts,), 2, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(31)
    G = _dev(rng.uniform(-1, 1, (npts, 6)))
    F = _dev(synth.field(S)).requires_grad_()
    fi = torch.zeros((npts, 6), dtype=torch.float64, device="cuda")
    out = hip.differentiable_fit_cloud(2, 2, S_d, F, hoods, fi, nk, knowns, wm)
    ref_out = fi.clone()
    hip.fit_cloud_device(2, 2, S_d, F.detach(), hoods, ref_out, nk, knowns, wm)
    assert torch.equal(_bits(out.detach()), _bits(ref_out))
    (out * G).sum().backward()
    # the per-slot gradients are the dense route's bits (xk = S[hoods])
    slots = _nan(npts, Kn)
    hip.fit_cloud_adjoint_device(2, 2, S_d, hoods, nk, knowns, wm, G, slots=slots, grad_fi=False)
    assert hip.last_kernel() == "adjoint-lane"
    safe = torch.where(hoods >= 0, hoods, torch.zeros_like(hoods)).long()
    dense, _ = hip.fit_many_adjoint_device(2, 2, S_d[safe].contiguous(), nk, S_d, knowns, wm, G, grad_fi=False)
    torch.cuda.synchronize()
    assert torch.equal(_bits(slots), _bits(dense))
    # F.grad against a float64 numpy scatter: index_add_'s order is not fixed, so per point 64 eps sum|contributions|, 64 being the
    # most slots one point receives contributions from in these clouds (asserted)
    sl, hd, nkh = slots.cpu().numpy(), hoods.cpu().numpy(), nk.cpu().numpy()
    want, mag, count = np.zeros(npts), np.zeros(npts), np.zeros(npts, np.int64)
    for j in range(npts):
        m = int(nkh[j])
        np.add.at(want, hd[j, :m], sl[j, :m]); np.add.at(mag, hd[j, :m], np.abs(sl[j, :m])); np.add.at(count, hd[j, :m], 1)
    assert count.max() <= 64
    assert np.all(np.abs(F.grad.cpu().numpy() - want) <= 64 * np.finfo(np.float64).eps * mag)


# ---- 6. capture ----

def test_forward_and_adjoint_replay_from_one_graph(hip):
    """fit_many_device and the adjoint recorded as one chain on one stream; replayed twice with new g: the eager results' bits."""
    import torch
    c = _synthetic(2, 2, 32, 200, 1, seed=41)
    rng = np.random.default_rng(42)
    t = {k: _dev(c[k]) for k in ("xk", "nk", "xi", "knowns", "wm")}
    fk = _dev(rng.uniform(-1, 1, (200, 32)))
    fi0 = _dev(rng.uniform(-1, 1, (200, 6)))
    fi, g = fi0.clone(), _dev(c["g"])
    gfk, gfi = _nan(200, 32), _nan(200, 6)

    def step():
        fi.copy_(fi0)
        hip.fit_many_device(2, 2, t["xk"], fk, t["nk"], t["xi"], fi, t["knowns"], t["wm"])
        hip.fit_many_adjoint_device(2, 2, t["xk"], t["nk"], t["xi"], t["knowns"], t["wm"], g, grad_fk=gfk, grad_fi=gfi)

    step()                                                            # warm-up outside the capture
    torch.cuda.synchronize()
    gfk.fill_(-7.0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        step()
    torch.cuda.synchronize()
    assert float(gfk.min()) == -7.0 and float(gfk.max()) == -7.0      # captured, not run
    for seed in (1, 2):
        g.copy_(_dev(np.random.default_rng(seed).uniform(-1, 1, (200, 6))))
        graph.replay()
        torch.cuda.synchronize()
        got = (fi.clone(), gfk.clone(), gfi.clone())
        gfk.fill_(-7.0); gfi.fill_(-7.0)
        step()
        torch.cuda.synchronize()
        for a, b in zip(got, (fi, gfk, gfi)):
            assert torch.equal(_bits(a), _bits(b))
