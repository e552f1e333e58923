"""CPU-only checks around the fit's adjoint (wlsqm.hip.fit_many_adjoint_device and friends): the oracle-built reference answer of
tests/_adjoint_ref.py against the real reference's golden sensitivities (which gives the fp64 noise floor N the GPU bar is built
from), the identity the kernel uses for the known columns, and the host-side surface (names, argument checks, header)."""
import os
import re

import numpy as np
import pytest

import _adjoint_ref as R
import _cases as K
import _parity as P
from _device_helpers import OnDevice as _OnDevice

ROOT = K.ROOT


@pytest.fixture(scope="module")
def floors():
    from oracle import oracle
    oracle.lib()
    return {dim: R.noise_floor(dim) for dim in (1, 2, 3)}


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_oracle_and_golden_sensitivities_give_the_same_grad_fk(floors, dim):
    """(a) grad_fk from the ORACLE's sens and from the REAL reference's golden sens, contracted with the same g: their per-case distance
    over the case's scale s[j] is the fp64 noise floor N of this quantity (printed).  "Agree" is the project's own tolerance: two fp64
    statements of the same algorithm (they differ in LAPACK's summation order only) within TOL per case.  Only cases with fewer neighbours than unknowns + 2 are left out, no more than the existing
    suites skip on the same fixture."""
    N, x = floors[dim]
    print("adjoint noise floor, sweep_%dd: N = %.3e over %d cases (%d left out of %d covered)"
          % (dim, N, int(x["use"].sum()), int((x["cov"] & ~x["ok"]).sum()), int(x["cov"].sum())))
    assert np.isfinite(N) and N <= P.TOL
    assert np.allclose(x["ref"]["s"][x["use"]], x["gold_s"][x["use"]], rtol=1e-6)
    assert (~x["ok"]).mean() <= (~x["suite"]).mean()
    assert x["use"].sum() >= 0.5 * x["cov"].sum()
    # the padding of a ragged row takes no part
    d = x["d"]
    live = np.arange(d["fk"].shape[1])[None, :] < d["nk"][:, None]
    assert np.all(x["ref"]["grad_fk"][~live] == 0.0) and np.all(x["gold_fk"][~live] == 0.0)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_known_columns_identity(floors, dim):
    """(b) grad_fi[a] = g[a] - sum_k c_k[a] grad_fk[k] for a true known a (what the kernel's second pass produces) against the helper's
    independent construction (the oracle fit of fk = 0 from fi = e_a); g[a] for a dropped DOF and 0 for an unknown."""
    N, x = floors[dim]
    d, g, ref = x["d"], x["g"], x["ref"]
    sums = R.monomial_sums(dim, d["order"], d["xk"], d["nk"], d["xi"], ref["grad_fk"])
    bar = P.TOL + P.NOISE_MULT * N
    checked = 0
    for j in np.where(x["use"])[0]:
        no = K.NDOF[dim][int(d["order"][j])]
        kn = int(d["knowns"][j])
        nun = R.unknowns(dim, d["order"][j], kn)
        free = [a for a in range(no) if not (kn >> a) & 1]
        for a in range(no):
            if (kn >> a) & 1:
                want = g[j, a] - sums[j, a]
                checked += 1
            elif a in free[nun:]:
                want = g[j, a]                                        # dropped by stray high bits: leaves the fit as it came in
            else:
                want = 0.0
            assert abs(ref["grad_fi"][j, a] - want) <= bar * ref["s"][j], (dim, j, a, ref["grad_fi"][j, a], want)
    assert checked > 20


def test_the_four_names_exist():
    """(c) the explicit adjoints and the autograd wrappers are part of wlsqm.hip (and not of the reference-shaped surface)."""
    import wlsqm
    import wlsqm.hip as h
    for name in ("fit_many_adjoint_device", "fit_cloud_adjoint_device", "differentiable_fit_many", "differentiable_fit_cloud"):
        assert callable(getattr(h, name)) and name in h.__all__
        assert not hasattr(wlsqm, name)


def _args(n=4, K_=7, dim=2, no=6):
    import torch
    g = torch.Generator().manual_seed(0)
    t = dict(xk=torch.rand((n, K_, dim), dtype=torch.float64, generator=g), nk=torch.full((n,), K_, dtype=torch.int32),
             xi=torch.zeros((n, dim), dtype=torch.float64), knowns=torch.zeros((n,), dtype=torch.int64),
             weighting_method=torch.full((n,), 2, dtype=torch.int32), g=torch.ones((n, no), dtype=torch.float64))
    return t


def test_adjoint_argument_validation():
    """(c) the checks of fit_many_device, with its messages, on the adjoint's arguments."""
    import wlsqm.hip as h
    t = _args()
    with pytest.raises(ValueError, match="must be a device"):
        h.fit_many_adjoint_device(2, 2, **t)
    dev = {k: _OnDevice(v) for k, v in t.items()}
    with pytest.raises(ValueError, match="dtype mismatch"):
        h.fit_many_adjoint_device(2, 2, **dict(dev, nk=_OnDevice(t["nk"].long())))
    with pytest.raises(ValueError, match="dtype mismatch"):
        h.fit_many_adjoint_device(2, 2, **dict(dev, knowns=_OnDevice(t["knowns"].int())))
    with pytest.raises(ValueError, match="dtype mismatch"):
        h.fit_many_adjoint_device(2, 2, **dict(dev, xk=_OnDevice(t["xk"].float())))
    with pytest.raises(ValueError, match="dtype mismatch"):
        h.fit_many_adjoint_device(2, 2, **dict(dev, g=_OnDevice(t["g"].float())))
    with pytest.raises(ValueError, match="wrong number of dimensions"):
        h.fit_many_adjoint_device(2, 2, **dict(dev, xk=_OnDevice(t["xk"][:, :, 0])))
    with pytest.raises(ValueError, match="not contiguous in the same dimension"):
        h.fit_many_adjoint_device(2, 2, **dict(dev, g=_OnDevice(t["g"].repeat(1, 2)[:, ::2])))
    with pytest.raises(ValueError, match="columns"):
        h.fit_many_adjoint_device(2, 2, **dict(dev, g=_OnDevice(t["g"][:, :5])))
    with pytest.raises(ValueError, match="rows"):
        h.fit_many_adjoint_device(2, 2, **dict(dev, g=_OnDevice(t["g"][:3])))
    with pytest.raises(ValueError, match="order must be"):
        h.fit_many_adjoint_device(2, 5, **dev)
    t3 = _args(dim=3, no=20)
    with pytest.raises(ValueError, match=r"unsupported \(dimension, order\)"):
        h.fit_many_adjoint_device(3, 3, **{k: _OnDevice(v) for k, v in t3.items()})
    with pytest.raises(ValueError, match="integer order"):
        h.fit_many_adjoint_device(2, _OnDevice(t["nk"]), **dev)
    with pytest.raises(ValueError, match="geometry is not differentiable"):
        h.differentiable_fit_many(2, 2, t["xk"].clone().requires_grad_(), t["g"], t["nk"], t["xi"], t["g"], t["knowns"], t["weighting_method"])


def test_both_symbols_are_declared_in_the_header():
    hdr = open(os.path.join(ROOT, "include", "wlsqm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("wlsqm_hip_fit_adjoint_device", "wlsqm_hip_fit_cloud_adjoint_device"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
