"""GPU tests of the adjoint of the prepared solve (ExpertSolver.solve_adjoint_device / solve_many_adjoint_device and the autograd
wrappers wlsqm.hip.differentiable_solve / differentiable_solve_many; csrc/solve_op.hip, csrc/expert.hip).  Criterion everywhere: per case
and field e_j = ||cand_j - ref_j||_inf / s[j] <= TOL + NOISE_MULT * N(dim) against tests/_adjoint_ref.py evaluated with g[r], with the
project's TOL and NOISE_MULT (tests/_parity.py) and N recomputed from the golden sweeps as tests/test_gpu_adjoint.py does.  The cases
are those of test_gpu_round2.py::test_solve_many_operator_path (tests/_solve_adjoint_cases.py): 333 cases, ragged nk within 7 of K,
case 7 fully known, mixed weightings, every case with at least unknowns + 2 neighbours (asserted there)."""
import numpy as np
import pytest

import _adjoint_ref as R
import _cases as K
import _parity as P
import _solve_adjoint_cases as SA
from _device_helpers import bits as _bits, dev as _dev, nan as _nan

pytestmark = pytest.mark.gpu

SWITCH = "WLSQM_HIP_SOLVE_ADJOINT"
OP_KERNEL = "solve-op-adjoint-mfma"
GEOMETRIC = ("adjoint-rows", "adjoint-lane")


@pytest.fixture(scope="module")
def wlsqm():
    import wlsqm as W
    from wlsqm import _binding
    assert _binding.lib().wlsqm_hip_device_count() >= 1, "no HIP device: the GPU tests need a real MI355X"
    return W


@pytest.fixture(scope="module")
def hip(wlsqm):
    import wlsqm.hip as h
    return h


@pytest.fixture(scope="module")
def floors():
    """dim -> N of the reference sweeps, computed once and shared."""
    return {dim: R.noise_floor(dim)[0] for dim in (1, 2, 3)}


def _bar(floors, dim):
    return P.TOL + P.NOISE_MULT * floors[dim]


def _solver(wlsqm, c, **kw):
    s = wlsqm.ExpertSolver(dimension=c["dim"], nk=c["nk"], order=c["orders"], knowns=c["knowns"], weighting_method=c["wm"], **kw)
    s.prepare(xi=c["xi"], xk=c["xk"])
    return s


def _check(c, r_lo, gfk, gfi, bar, what):
    """gfk (R, n, K), gfi (R, n, >= no) numpy, fields r_lo .. r_lo + R of the problem: the reference and the exact properties."""
    n, no, Kn = c["n"], c["no"], c["K"]
    nf = gfk.shape[0]
    ref_fk, ref_fi, s, g = (c[k][r_lo:r_lo + nf] for k in ("ref_fk", "ref_fi", "s", "g"))
    assert not np.isnan(gfk).any(), what                              # every grad_fk slot is written
    live = np.arange(Kn)[None, :] < c["nk"][:, None]
    assert np.all(gfk[:, ~live] == 0.0), what                         # the padding: exact zeros
    assert np.all(gfk[:, 7] == 0.0), what                             # the fully known case
    assert np.array_equal(gfi[:, 7, :no], g[:, 7]), what              # ... passes g through, bit for bit
    assert np.all(np.isnan(gfi[:, :, no:])), what                     # columns beyond `no` are untouched
    U, _, D = SA.classes(no, c["mask"])
    rest = np.arange(n) != 7
    assert np.all(gfi[:, rest][:, :, U] == 0.0), what                 # an unknown's incoming value is never read
    assert np.array_equal(gfi[:, rest][:, :, D], g[:, rest][:, :, D]), what     # dropped DOFs leave as they came in
    with np.errstate(invalid="ignore"):
        e_fk = np.abs(gfk - ref_fk).max(axis=2) / s
        e_fi = np.abs(gfi[:, :, :no] - ref_fi).max(axis=2) / s
    print("%s: bar %.3e, grad_fk max e %.3e, grad_fi max e %.3e over %d fields x %d cases" % (what, bar, e_fk.max(), e_fi.max(), nf, n))
    assert e_fk.max() <= bar and e_fi.max() <= bar, (what, e_fk.max(), e_fi.max(), bar)


def _adjoint(s, c, r_lo, nf, wide_fi=2):
    import torch
    g = _dev(c["g"][r_lo:r_lo + nf])
    gfk, gfi = _nan(nf, c["n"], c["K"]), _nan(nf, c["n"], c["no"] + wide_fi)
    s.solve_many_adjoint_device(g, grad_fk=gfk, grad_fi=gfi)
    torch.cuda.synchronize()
    return gfk, gfi


# ---- 1. the operator route, forced ----

SHAPES = [
    # dim, order, K, knowns
    (2, 2, 32, 0),
    (2, 2, 32, 1),
    (3, 2, 40, 0b10001),                                              # a k-block half inside the operator row
    (3, 2, 36, 0),                                                    # K < KP = 40
    (2, 4, 64, 1),                                                    # 15 unknowns
    (2, 3, 24, 0b1011),                                               # three knowns, 1.5 k-blocks
    (2, 2, 30, 1),                                                    # pad columns
    (2, 1, 10, 0),                                                    # KP = 16
    (2, 2, 62, 0),
    (1, 2, 12, 0),
]
IDS = ["%dd-o%d-K%d-kn%d" % s for s in SHAPES]
STACK = 37


def _problem(i):
    dim, order, Kn, knowns = SHAPES[i]
    return SA.problem(dim, order, Kn, knowns, nfields=70 if i == 0 else STACK)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_operator_route(wlsqm, hip, floors, monkeypatch, i):
    c = _problem(i)
    s = _solver(wlsqm, c)
    monkeypatch.setenv(SWITCH, "o")
    for nf in (1, 5, 16, 37) + ((70,) if i == 0 else ()):             # 70: more fields than any one loop iteration handles
        gfk, gfi = _adjoint(s, c, 0, nf)
        assert hip.last_kernel() == OP_KERNEL, hip.last_kernel()
        _check(c, 0, gfk.cpu().numpy(), gfi.cpu().numpy(), _bar(floors, c["dim"]), "%s operator R=%d" % (IDS[i], nf))
    s.close()


def test_operator_route_dropped_dofs(wlsqm, hip, floors, monkeypatch):
    """One stray high mask bit drops the last unknown: grad_fi is g there, bit for bit (checked in _check), and no knowns' term is lost."""
    c = SA.problem(2, 2, 32, (1 << 9) | 2, nfields=5)
    s = _solver(wlsqm, c)
    monkeypatch.setenv(SWITCH, "o")
    gfk, gfi = _adjoint(s, c, 0, 5)
    assert hip.last_kernel() == OP_KERNEL
    assert SA.classes(6, c["mask"])[2] == [5]
    _check(c, 0, gfk.cpu().numpy(), gfi.cpu().numpy(), _bar(floors, 2), "dropped DOF")
    # grad_fi not wanted: grad_fk has the same bits
    import torch
    gfk2 = _nan(5, c["n"], 32)
    out = s.solve_many_adjoint_device(_dev(c["g"][:5]), grad_fk=gfk2, grad_fi=False)
    torch.cuda.synchronize()
    assert out[1] is None and out[0] is gfk2 and torch.equal(_bits(gfk2), _bits(gfk))
    s.close()


# ---- 2. stack independence ----

@pytest.mark.parametrize("i", [1, 4], ids=[IDS[1], IDS[4]])
def test_a_field_does_not_depend_on_its_stack(wlsqm, hip, monkeypatch, i):
    import torch
    c = _problem(i)
    s = _solver(wlsqm, c)
    monkeypatch.setenv(SWITCH, "o")
    full_fk, full_fi = _adjoint(s, c, 0, STACK)
    guest = wlsqm.ExpertSolver(dimension=c["dim"], nk=c["nk"], order=c["orders"], knowns=c["knowns"], weighting_method=c["wm"], host=s)
    guest.prepare(xi=c["xi"], xk=c["xk"])
    for r in (0, 17, 36):
        lo = min(r, STACK - 5)
        for solver, r_lo, nf in ((s, lo, 5), (s, r, 1), (guest, lo, 5)):
            gfk, gfi = _adjoint(solver, c, r_lo, nf)
            assert hip.last_kernel() == OP_KERNEL
            assert torch.equal(_bits(gfk[r - r_lo]), _bits(full_fk[r])) and torch.equal(_bits(gfi[r - r_lo]), _bits(full_fi[r]))
    guest.close(); s.close()


# ---- 3. the geometric route ----

@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_geometric_route(wlsqm, hip, floors, monkeypatch, i):
    import torch
    c = _problem(i)
    s = _solver(wlsqm, c)
    monkeypatch.setenv(SWITCH, "g")
    gfk, gfi = _adjoint(s, c, 0, 3)
    assert hip.last_kernel() in GEOMETRIC, hip.last_kernel()
    _check(c, 0, gfk.cpu().numpy(), gfi.cpu().numpy(), _bar(floors, c["dim"]), "%s geometric R=3" % IDS[i])
    if c["no"] <= 10:
        # the bits of the fit's adjoint on the arrays the solver was prepared from
        t = {k: _dev(c[k]) for k in ("xk", "nk", "xi", "knowns", "wm")}
        for r in range(3):
            fk_x, fi_x = hip.fit_many_adjoint_device(c["dim"], c["order"], t["xk"], t["nk"], t["xi"], t["knowns"], t["wm"], _dev(c["g"][r]))
            torch.cuda.synchronize()
            assert torch.equal(_bits(gfk[r]), _bits(fk_x)) and torch.equal(_bits(gfi[r, :, :c["no"]]), _bits(fi_x))
    s.close()


@pytest.mark.parametrize("what", ["K7", "five-knowns", "mixed-orders"])
def test_shapes_without_an_operator_take_the_geometric_route_by_default(wlsqm, hip, floors, monkeypatch, what):
    import torch
    monkeypatch.delenv(SWITCH, raising=False)
    nf = 16                                                           # a stack the default dispatch would give the operator, had the shape one
    if what == "K7":
        c = SA.problem(2, 1, 7, 0, nfields=nf)
    elif what == "five-knowns":
        c = SA.problem(2, 2, 32, 0b11111, nfields=nf)
    else:
        c = SA.geometry(2, 2, 32, 0)
        c["orders"] = np.where(np.arange(c["n"]) % 3 == 0, 1, 2).astype(np.int32)
        c["knowns"] = np.where(c["orders"] == 1, c["knowns"] & 0b111, c["knowns"])     # case 7 (order 2) keeps its full mask
        assert R.resolvable(2, c["orders"], c["nk"], c["knowns"])[0].all()
        c["g"] = np.random.default_rng(5).uniform(-1, 1, (nf, c["n"], 6))
    s = _solver(wlsqm, c)
    g = _dev(c["g"])
    gfk, gfi = _nan(nf, c["n"], c["K"]), _nan(nf, c["n"], c["no"] + 2)
    s.solve_many_adjoint_device(g, grad_fk=gfk, grad_fi=gfi)
    torch.cuda.synchronize()
    assert hip.last_kernel() in GEOMETRIC, hip.last_kernel()
    if what != "mixed-orders":
        _check(c, 0, gfk.cpu().numpy(), gfi.cpu().numpy(), _bar(floors, 2), what)
    else:
        gfk, gfi = gfk.cpu().numpy(), gfi.cpu().numpy()
        assert not np.isnan(gfk).any()
        for r in (0, nf - 1):
            ref = R.adjoint_ref(2, c["orders"], c["xk"], c["nk"], c["xi"], c["knowns"], c["wm"], c["g"][r])
            for j in range(c["n"]):
                no = K.NDOF[2][int(c["orders"][j])]
                assert np.abs(gfk[r, j] - ref["grad_fk"][j]).max() <= _bar(floors, 2) * ref["s"][j]
                assert np.abs(gfi[r, j, :no] - ref["grad_fi"][j, :no]).max() <= _bar(floors, 2) * ref["s"][j]
                assert np.all(np.isnan(gfi[r, j, no:]))               # columns beyond the case's own number of DOFs are untouched
    s.close()


def test_unsupported_solvers_raise(wlsqm, hip):
    c = SA.geometry(3, 3, 40, 0, n=8)
    s = _solver(wlsqm, c)
    with pytest.raises(ValueError, match=r"unsupported \(dimension, order\)"):
        s.solve_many_adjoint_device(_nan(2, 8, 20))
    with pytest.raises(ValueError, match=r"unsupported \(dimension, order\)"):
        s.solve_adjoint_device(_nan(8, 20))
    s.close()
    c = SA.geometry(2, 2, 32, 0, n=8)
    from wlsqm.fitter import defs
    s = _solver(wlsqm, c, algorithm=defs.ALGO_ITERATIVE)
    with pytest.raises(ValueError, match="ALGO_ITERATIVE"):
        s.solve_many_adjoint_device(_nan(2, 8, 6))
    s.close()


# ---- 4. dot-product test against the existing forward ----

def test_dot_product_against_the_operator_forward(wlsqm, hip, floors, monkeypatch):
    import torch
    c = _problem(1)                                                   # 2D order 2, 32 neighbours, F known
    nf, n = 16, c["n"]
    s = _solver(wlsqm, c)
    rng = np.random.default_rng(44)
    fk0, fi0 = _dev(rng.uniform(-1, 1, (nf, n, 32))), _dev(rng.uniform(-1, 1, (nf, n, 6)))
    v, u = _dev(rng.uniform(-1, 1, (nf, n, 32))), _dev(rng.uniform(-1, 1, (nf, n, 6)))
    G = _dev(c["g"][:nf])
    monkeypatch.setenv("WLSQM_HIP_SOLVE_MANY", "op")
    monkeypatch.setenv(SWITCH, "o")

    def solve(fk, fi):
        out = fi.clone()
        s.solve_many_device(fk, out)
        assert hip.last_kernel() == "solve-op-mfma"
        return out

    base = solve(fk0, fi0)
    gfk, gfi = s.solve_many_adjoint_device(G)
    assert hip.last_kernel() == OP_KERNEL
    lhs_terms = (solve(fk0 + v, fi0 + u) - base) * G
    rhs_terms = torch.cat([(v * gfk).reshape(-1), (u * gfi).reshape(-1)])
    lhs, rhs = float(lhs_terms.sum()), float(rhs_terms.sum())
    scale = float(lhs_terms.abs().sum() + rhs_terms.abs().sum())
    print("dot-product test: lhs %.15e rhs %.15e, |lhs - rhs| / sum|terms| = %.3e" % (lhs, rhs, abs(lhs - rhs) / scale))
    assert abs(lhs - rhs) <= 2.0 * _bar(floors, 2) * scale
    s.close()


# ---- 5. autograd ----

def test_autograd_through_the_prepared_solver(wlsqm, hip, monkeypatch):
    import torch
    c = _problem(1)
    nf, n = 5, c["n"]
    s = _solver(wlsqm, c)
    assert s.prepare_operator()
    monkeypatch.setenv(SWITCH, "o")
    rng = np.random.default_rng(45)
    fk0, fi0 = _dev(rng.uniform(-1, 1, (nf, n, 32))), _dev(rng.uniform(-1, 1, (nf, n, 6)))
    G = _dev(c["g"][:nf])
    gfk_x, gfi_x = s.solve_many_adjoint_device(G)
    assert hip.last_kernel() == OP_KERNEL
    ref = fi0.clone()
    s.solve_many_device(fk0, ref)
    fk, fi = fk0.clone().requires_grad_(), fi0.clone().requires_grad_()
    out = hip.differentiable_solve_many(s, fk, fi)
    assert torch.equal(_bits(out.detach()), _bits(ref))               # the forward is solve_many_device's bits
    assert torch.equal(_bits(fi.detach()), _bits(fi0))                # fi itself is not written
    (out * G).sum().backward()
    assert torch.equal(_bits(fk.grad), _bits(gfk_x)) and torch.equal(_bits(fi.grad), _bits(gfi_x))
    # only the gradient that is needed
    seen = []
    inner = s.solve_many_adjoint_device
    s.solve_many_adjoint_device = lambda g, **kw: (seen.append(kw["grad_fi"]), inner(g, **kw))[1]
    fk = fk0.clone().requires_grad_()
    out = hip.differentiable_solve_many(s, fk, fi0)
    (out * G).sum().backward()
    assert seen == [False] and torch.equal(_bits(fk.grad), _bits(gfk_x))
    out = hip.differentiable_solve_many(s, fk0, fi0)
    assert not out.requires_grad
    del s.solve_many_adjoint_device
    # a wider fk, more rows and columns of fi than the solve touches: zeros / g passed through
    fkw = torch.zeros((nf, n + 2, 38), dtype=torch.float64, device="cuda"); fkw[:, :n, :32] = fk0
    fiw = torch.zeros((nf, n + 2, 8), dtype=torch.float64, device="cuda"); fiw[:, :n, :6] = fi0
    Gw = _dev(rng.uniform(-1, 1, (nf, n + 2, 8))); Gw[:, :n, :6] = G
    refw = fiw.clone()
    s.solve_many_device(fkw, refw)                                    # (rows at another pitch may take another forward kernel: its bits)
    fkw.requires_grad_(); fiw.requires_grad_()
    out = hip.differentiable_solve_many(s, fkw, fiw)
    assert torch.equal(_bits(out.detach()), _bits(refw))
    (out * Gw).sum().backward()
    assert torch.equal(_bits(fkw.grad[:, :n, :32]), _bits(gfk_x))
    assert float(fkw.grad[:, :, 32:].abs().max()) == 0.0 and float(fkw.grad[:, n:].abs().max()) == 0.0
    assert torch.equal(_bits(fiw.grad[:, :n, :6]), _bits(gfi_x))
    assert torch.equal(_bits(fiw.grad[:, n:]), _bits(Gw[:, n:])) and torch.equal(_bits(fiw.grad[:, :, 6:]), _bits(Gw[:, :, 6:]))
    # one field
    g1x, i1x = s.solve_adjoint_device(G[0])
    ref1 = fi0[0].clone()
    s.solve_device(fk0[0], ref1)
    fk, fi = fk0[0].clone().requires_grad_(), fi0[0].clone().requires_grad_()
    out = hip.differentiable_solve(s, fk, fi)
    assert torch.equal(_bits(out.detach()), _bits(ref1))
    (out * G[0]).sum().backward()
    assert torch.equal(_bits(fk.grad), _bits(g1x)) and torch.equal(_bits(fi.grad), _bits(i1x))
    s.close()


# ---- 6. capture ----

def _capture_and_replay(s, hip, c, nf, expect):
    import torch
    n = c["n"]
    rng = np.random.default_rng(46)
    fk = _dev(rng.uniform(-1, 1, (nf, n, 32)))
    fi0 = _dev(rng.uniform(-1, 1, (nf, n, 6)))
    fi, g = fi0.clone(), _dev(c["g"][:nf])
    gfk, gfi = _nan(nf, n, 32), _nan(nf, n, 6)

    def step():
        fi.copy_(fi0)
        s.solve_many_device(fk, fi)
        s.solve_many_adjoint_device(g, grad_fk=gfk, grad_fi=gfi)

    gfk.fill_(-7.0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        step()
    assert hip.last_kernel() in expect, hip.last_kernel()
    torch.cuda.synchronize()
    assert float(gfk.min()) == -7.0 and float(gfk.max()) == -7.0      # captured, not run
    return graph, step, g, (fi, gfk, gfi)


def test_forward_and_adjoint_replay_from_one_graph(wlsqm, hip, monkeypatch):
    import torch
    c = _problem(1)
    nf = 5
    # (a) with the operator present: both calls only enqueue kernels
    s = _solver(wlsqm, c)
    assert s.prepare_operator()
    monkeypatch.setenv("WLSQM_HIP_SOLVE_MANY", "op")
    monkeypatch.setenv(SWITCH, "o")
    warm = _adjoint(s, c, 0, nf)                                      # warm-up outside the capture
    fiw = _dev(np.zeros((nf, c["n"], 6))); s.solve_many_device(_dev(np.zeros((nf, c["n"], 32))), fiw)
    torch.cuda.synchronize()
    graph, step, g, outs = _capture_and_replay(s, hip, c, nf, (OP_KERNEL,))
    for seed in (1, 2):
        g.copy_(_dev(np.random.default_rng(seed).uniform(-1, 1, tuple(g.shape))))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in outs]
        outs[1].fill_(-7.0); outs[2].fill_(-7.0)
        step()
        torch.cuda.synchronize()
        assert hip.last_kernel() == OP_KERNEL
        for a, b in zip(got, outs):
            assert torch.equal(_bits(a), _bits(b))
    s.close()
    # (b) a solver without an operator: the default dispatch wants one for this stack, but never builds it while capturing
    s = _solver(wlsqm, c)
    monkeypatch.delenv("WLSQM_HIP_SOLVE_MANY")
    monkeypatch.setenv(SWITCH, "g")
    _adjoint(s, c, 0, nf)                                             # warm-up: the geometric route builds nothing
    fiw = _dev(np.zeros((nf, c["n"], 6))); s.solve_many_device(_dev(np.zeros((nf, c["n"], 32))), fiw)
    torch.cuda.synchronize()
    monkeypatch.delenv(SWITCH)
    graph, step, g, outs = _capture_and_replay(s, hip, c, nf, GEOMETRIC)
    monkeypatch.setenv(SWITCH, "g")
    for seed in (3, 4):
        g.copy_(_dev(np.random.default_rng(seed).uniform(-1, 1, tuple(g.shape))))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in outs]
        outs[1].fill_(-7.0); outs[2].fill_(-7.0)
        step()
        torch.cuda.synchronize()
        assert hip.last_kernel() in GEOMETRIC
        for a, b in zip(got, outs):
            assert torch.equal(_bits(a), _bits(b))
    s.close()
