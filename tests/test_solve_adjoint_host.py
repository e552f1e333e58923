"""CPU-only checks around the adjoint of the prepared solve (ExpertSolver.solve_adjoint_device / solve_many_adjoint_device,
wlsqm.hip.differentiable_solve / differentiable_solve_many; csrc/solve_op.hip): the C and Python surface, the argument checks that
need no device, and a numpy rehearsal of the operator route (the transposed stored operator and the correction block T) against
tests/_adjoint_ref.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import _adjoint_ref as R
import _cases as K
import _parity as P
import _solve_adjoint_cases as SA
from _device_helpers import OnDevice as _OnDevice

ROOT = K.ROOT
NAME = "wlsqm_hip_expert_solve_adjoint_device"


def test_header_declares_and_library_exports_the_entry_point():
    from wlsqm import _binding
    if not os.path.exists(_binding.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    hdr = open(os.path.join(ROOT, "include", "wlsqm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, hdr)
    assert m, NAME
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 13 and args[0] == "wlsqm_expert* h" and args[1] == "void* stream" and args[2] == "int64_t nrhs"
    assert args[9] == "int64_t gfk_slots"
    assert hasattr(C.CDLL(_binding.LIB_PATH), NAME)


def test_the_four_python_names_exist():
    import wlsqm
    import wlsqm.hip as h
    from wlsqm.fitter.expert import ExpertSolver
    for name in ("solve_adjoint_device", "solve_many_adjoint_device"):
        sig = inspect.signature(getattr(ExpertSolver, name))
        assert list(sig.parameters) == ["self", "g", "grad_fk", "grad_fi", "stream"]
        assert all(sig.parameters[p].default is None for p in ("grad_fk", "grad_fi", "stream"))
    for name in ("differentiable_solve", "differentiable_solve_many"):
        sig = inspect.signature(getattr(h, name))
        assert list(sig.parameters) == ["solver", "fk", "fi", "stream"] and sig.parameters["stream"].default is None
        assert name in h.__all__ and not hasattr(wlsqm, name)


def _solver(ready=True, n=4, max_nk=8, no=6):
    """An ExpertSolver shell without device state: what the argument checks look at."""
    from wlsqm.fitter.expert import ExpertSolver
    s = ExpertSolver.__new__(ExpertSolver)
    s._handle = None; s._tree = None; s._tree_points = None
    s.ready, s.ncases, s._max_nk, s._max_no, s._device = ready, n, max_nk, no, 0
    s.order = np.full(n, 2, np.int32)
    return s


def test_argument_checks_without_a_device():
    import torch
    import wlsqm.hip as h
    n, Kn, no, R_ = 4, 8, 6, 3
    s = _solver()
    g2, g3 = torch.ones((n, no), dtype=torch.float64), torch.ones((R_, n, no), dtype=torch.float64)
    fk3, fk2 = torch.ones((R_, n, Kn), dtype=torch.float64), torch.ones((n, Kn), dtype=torch.float64)
    D = _OnDevice
    for call, g, rank in ((s.solve_adjoint_device, g2, 2), (s.solve_many_adjoint_device, g3, 3)):
        with pytest.raises(ValueError, match="g must be a %d-D float64 device tensor" % rank):
            call(g)                                                   # a host tensor
        with pytest.raises(ValueError, match="g must be a %d-D float64 device tensor" % rank):
            call(D(g.float()))                                        # dtype
        with pytest.raises(ValueError, match="g must be a %d-D float64 device tensor" % rank):
            call(D(g[0]))                                             # rank
        with pytest.raises(ValueError, match="contiguous last axis"):
            call(D(g.repeat_interleave(2, dim=-1)[..., ::2]))         # contiguity
        with pytest.raises(ValueError, match="g has 5 columns, need at least 6"):
            call(D(g[..., :5]))                                       # too few columns
        with pytest.raises(ValueError, match="too small"):
            call(D(g[..., :3, :]))                                    # too few rows
        with pytest.raises(ValueError, match="too small"):
            call(D(g), grad_fk=D(torch.ones(g.shape[:-1] + (Kn - 1,), dtype=torch.float64)))
        with pytest.raises(ValueError, match="grad_fi has 5 columns"):
            call(D(g), grad_fi=D(g[..., :5].contiguous()))
        with pytest.raises(ValueError, match="grad_fk must be a %d-D float64" % rank):
            call(D(g), grad_fk=D(torch.ones(g.shape[:-1] + (Kn,), dtype=torch.float32)))
        with pytest.raises(ValueError, match="solver's device"):
            call(D(g))                                                # every check passed: the tensor is not on cuda:0 after all
    with pytest.raises(ValueError, match="same number"):
        s.solve_many_adjoint_device(D(g3), grad_fk=D(fk3[:2]))
    # the autograd wrappers: the messages of solve_device / solve_many_device
    with pytest.raises(ValueError, match="fk must be a 3-D float64 device tensor"):
        h.differentiable_solve_many(s, fk3, D(g3))
    with pytest.raises(ValueError, match="fi must be a 2-D float64 device tensor"):
        h.differentiable_solve(s, D(fk2), D(g2.float()))
    with pytest.raises(ValueError, match="same number"):
        h.differentiable_solve_many(s, D(fk3), D(g3[:2]))             # field counts that differ
    with pytest.raises(ValueError, match="fk/fi are too small"):
        h.differentiable_solve_many(s, D(fk3[:, :, :7]), D(g3))
    with pytest.raises(ValueError, match="fi has 5 columns, need at least 6"):
        h.differentiable_solve(s, D(fk2), D(g2[:, :5]))
    # an unprepared solver
    u = _solver(ready=False)
    for call, args in ((u.solve_adjoint_device, (D(g2),)), (u.solve_many_adjoint_device, (D(g3),)),
                       (h.differentiable_solve, (u, D(fk2), D(g2))), (h.differentiable_solve_many, (u, D(fk3), D(g3)))):
        with pytest.raises(RuntimeError, match="not in the ready state"):
            call(*args)


def test_switch_is_a_row_of_the_dispatch_table():
    text = open(os.path.join(ROOT, "python-wlsqm_amd", "csrc", "wlsqm_dispatch.hpp")).read()
    assert re.search(r"^//   WLSQM_HIP_SOLVE_ADJOINT +A/B +=g \| =o ", text, flags=re.M)


# ---- the operator route in numpy ----

@pytest.fixture(scope="module")
def floors():
    from oracle import oracle
    oracle.lib()
    return {dim: R.noise_floor(dim)[0] for dim in (2, 3)}


REHEARSAL = [(2, 2, 32), (3, 2, 40), (2, 3, 24)]


@pytest.mark.parametrize("dim,order,Kn", REHEARSAL)
@pytest.mark.parametrize("mask", ["none", "F", "0b1011", "stray"])
def test_operator_route_in_numpy(floors, dim, order, Kn, mask):
    """op (zero rows for knowns and dropped DOFs, zero columns from nk on) and T = op C[:, knowns] built from the oracle's sensitivities;
    op^T g and g[a_t] - T^T g against adjoint_ref's grad_fk / grad_fi, per case within TOL + NOISE_MULT * N."""
    no = K.NDOF[dim][order]
    knowns = {"none": 0, "F": 1, "0b1011": 0b1011, "stray": (1 << (no + 3)) | 2}[mask]
    c = SA.problem(dim, order, Kn, knowns, nfields=2, n=40)
    n, sens = c["n"], c["sens"]
    KP = (Kn + 7) // 8 * 8
    op = np.zeros((n, no, KP))
    split = [SA.classes(no, c["knowns"][j]) for j in range(n)]
    for j in range(n):
        U = split[j][0]
        m = int(c["nk"][j])
        op[j][U, :m] = sens[j, :m, :][:, U].T
    assert not np.isnan(op).any()
    # T[j, a, t] = sum_k op[j, a, k] c_k[a_t]
    T = np.zeros((n, no, 4))
    for a in range(no):
        sums = R.monomial_sums(dim, order, c["xk"], c["nk"], c["xi"], op[:, a, :Kn])
        for j in range(n):
            for t, at in enumerate(split[j][1][:4] if split[j][0] else []):
                T[j, a, t] = sums[j, at]
    bar = P.TOL + P.NOISE_MULT * floors[dim]
    worst = 0.0
    for r in range(c["g"].shape[0]):
        g = c["g"][r]
        gfk = np.einsum("jak,ja->jk", op, g)[:, :Kn]
        gfi = np.zeros((n, no))
        for j in range(n):
            U, Kt, Dr = split[j]
            if not U:
                gfi[j] = g[j]                                         # nothing to solve: the fit leaves fi as it came in
                continue
            gfi[j, Dr] = g[j, Dr]
            for t, at in enumerate(Kt):
                gfi[j, at] = g[j, at] - float(np.dot(T[j, :, t], g[j]))
        e_fk = np.abs(gfk - c["ref_fk"][r]).max(axis=1) / c["s"][r]
        e_fi = np.abs(gfi - c["ref_fi"][r]).max(axis=1) / c["s"][r]
        worst = max(worst, e_fk.max(), e_fi.max())
        assert e_fk.max() <= bar and e_fi.max() <= bar, (r, e_fk.max(), e_fi.max(), bar)
        live = np.arange(Kn)[None, :] < c["nk"][:, None]
        assert np.all(gfk[~live] == 0.0) and np.all(gfk[7] == 0.0)
    print("rehearsal %dD order %d K %d mask %s: worst e = %.3e, bar = %.3e" % (dim, order, Kn, mask, worst, bar))
