"""GPU tests of the fit's LINEAR OPERATOR on structured and adversarial neighbourhoods (tests/_adversarial.py, OP_FAMILIES): the
sensitivities sens[j, k, a] = d fi_a / d fk_k through `fit_many_device(..., sens=)`, and the three kernels that apply the operator's
transpose: `adjoint-lane` / `adjoint-rows` (csrc/fit_adjoint.hip; fit_many_adjoint_device, fit_cloud_adjoint_device) and
`solve-op-adjoint-mfma` (csrc/solve_op.hip; ExpertSolver.solve_many_adjoint_device).

Truth: `_parity.truth_operator_mp` (the operator in mpmath, one elimination per case) and `_parity.truth_adjoint_mp` (its transpose applied
to g, contracted in mpmath before anything is rounded).  Reference: the CPU oracle's sensitivities and the adjoint built from the oracle
(tests/_adjoint_ref.py).  Criteria, the project's own (tests/_parity.py, NOISE_MULT = 8, Q_FLOOR):
  (a) per family batch, the column criterion  E <= 1e-10 + 8 N  (sens: per DOF column over the live entries, `assert_parity`; gradients:
      per case in the case's scale s_j, N the oracle-built reference's worst case, `assert_scaled`);
  (b) per case,  max_j q_j(GPU) <= 8 max_j q_j(oracle) + Q_FLOOR,  q_j the case's error over eps kappa_j^2 (sens: in the column scale
      over the batch's live entries, `sens_q`; gradients: err / (s_j eps kappa_j^2), `grad_q`): one wrong lane cannot hide behind the
      worst-conditioned case of its batch.
Every family is a batch of A.N_OP = 96 cases (a full wave and a half-filled one, each holding several knowns / weighting kinds); the truths
of a shape are computed once per module, in worker processes that never touch the GPU.  3D order 4 is left out: an mpmath operator with
35 unknowns and 64 right-hand sides costs minutes, and its inverse comes from the same fit_rows.hip path that 3D order 3 runs.
"""
import numpy as np
import pytest

import _adjoint_ref as R
import _adversarial as A
import _parity as P
from _device_helpers import dev as _t, oracle, same_bits as _same_bits, wlsqm  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

N = A.N_OP
WORKERS = 12
UNTOUCHED = 777.0
# strict and accurate mode with sensitivities: the map's accurate section names `strict-rows` for every shape here, and the strict mode
# takes the same dispatch (launch_fit_strict, csrc/fit_strict.hip: a call with sensitivities is the row-per-lane kernel's)
STRICT_SENS_KERNEL = "strict-rows"
# the kernel of a dense launch with sensitivities per shape (the second entry of a line of profiles/dispatch_map_current.txt)
SENS_KERNEL = {(2, 2, 32): "tile1-extras", (3, 2, 40): "tile1-extras", (1, 4, 12): "tile1-extras", (2, 4, 64): "sens-apply",
               (3, 3, 64): "sens-apply"}
STAGED_SHAPES = ((2, 2, 32), (3, 2, 40))            # again under WLSQM_HIP_STAGE_SENS=a: csrc/fit_stage_iter.hip
ADJOINT_SHAPES = ((2, 2, 32), (2, 3, 30), (2, 4, 64), (3, 2, 40), (1, 2, 8), (1, 4, 12))
CLOUD_SHAPES = ((2, 2, 32), (3, 2, 40))
SOLVE_SHAPES = ((2, 2, 32), (3, 2, 40))
SOLVE_FAMILIES = ("aniso", "far", "grid", "collinear", "self", "tiny_edge", "huge_edge")
_ids = lambda s: "%dD-o%d-K%d" % s


def _full(shape, value):
    import torch
    return torch.full(shape, value, dtype=torch.float64, device="cuda")


_CACHE = {}


def _shape_data(oracle, shape):
    """All families of one shape: the batch, the operator's truth (S, J, kappa, masks, the adjoint of fields 0 and 2), the oracle's fit
    and sensitivities, and where the adjoint covers the shape the oracle-built adjoint of the same fields.  For the shapes whose
    sensitivities come with an fi from another kernel than the basic fit's, the mpmath truth of fi.  Computed once per module; nothing
    modifies it."""
    if shape in _CACHE:
        return _CACHE[shape]
    dim, order, K = shape
    step = 32
    per = N // step
    res = A.operators([(f, dim, order, K, N, lo, lo + step) for f in A.OP_FAMILIES for lo in range(0, N, step)], WORKERS)
    fits = None
    if SENS_KERNEL.get(shape) == "sens-apply":
        fits = A.truths([(f, dim, order, K, N, lo, lo + step) for f in A.OP_FAMILIES for lo in range(0, N, step)], WORKERS)
    out = {}
    for i, f in enumerate(A.OP_FAMILIES):
        b = A.op_batch(f, dim, order, K, N)
        b["T"] = A.operator_truth(f, dim, order, K, N, res[i * per:(i + 1) * per])
        fi, sens = b["fi0"].copy(), np.full((N, K, b["no"]), UNTOUCHED)
        oracle.fit_many(dim, b["xk"], b["fk"], b["nk"], b["xi"], fi, sens, 1, b["order_a"], b["kn"], b["wm"])
        assert np.isfinite(sens[b["T"]["live"]]).all() and np.isfinite(fi).all(), (f, shape)
        b["oracle_fi"], b["oracle_sens"] = fi, sens
        if fits is not None:
            b["truth_fi"] = np.concatenate([r[0] for r in fits[i * per:(i + 1) * per]])
            assert np.array_equal(np.concatenate([r[1] for r in fits[i * per:(i + 1) * per]]), b["T"]["kappa"])
        b["g"], b["ref"] = {}, {}
        if R.covered(dim, order):
            for field in A.OP_FIELDS:
                b["g"][field] = A.op_g(f, dim, order, K, N, field)
                ref = R.adjoint_ref(dim, order, b["xk"], b["nk"], b["xi"], b["kn"], b["wm"], b["g"][field], sens=sens)
                assert np.isfinite(ref["grad_fk"]).all() and np.isfinite(ref["grad_fi"]).all(), (f, shape)
                b["ref"][field] = ref
        out[f] = b
    _CACHE[shape] = out
    return out


def _what(route, b):
    return "%s, %s %dD order %d K %d" % (route, b["family"], b["dim"], b["order"], b["K"])


# ---- sensitivities -----------------------------------------------------------------------------------------------------------------

def _fit_with_sens(whip, b, mode=None):
    import torch
    fi, sens = _t(b["fi0"]), _full((N, b["K"], b["no"]), UNTOUCHED)
    whip.fit_many_device(b["dim"], b["order"], _t(b["xk"]), _t(b["fk"]), _t(b["nk"]), _t(b["xi"]), fi, _t(b["kn"]), _t(b["wm"]), sens=sens,
                         strict=mode)
    torch.cuda.synchronize()
    return fi.cpu().numpy(), sens.cpu().numpy(), whip.last_kernel()


def _check_sens(route, b, sens):
    """The pattern of untouched / NaN entries as the oracle's; criteria (a) and (b) over the live entries."""
    what, T, ora = _what(route, b), b["T"], b["oracle_sens"]
    assert np.array_equal(sens == UNTOUCHED, ora == UNTOUCHED), what + ": entries of unused slots or of dropped columns were written"
    assert np.array_equal(np.isnan(sens), np.isnan(ora)), what + ": NaN pattern of sens"
    qc, qo = P.sens_q(sens, T["S"], T["live"], T["kappa"]), P.sens_q(ora, T["S"], T["live"], T["kappa"])
    print("%-72s max q: gpu %.3g oracle %.3g" % (what, qc.max(), qo.max()))
    rows = np.arange(b["K"])[None, :] < b["nk"][:, None]
    P.assert_parity(sens[rows], ora[rows], np.where(T["live"], T["S"], np.nan)[rows], what)
    P.assert_q(qc, qo, T["kappa"], what)


def _check_fi(route, b, fi):
    what = _what(route, b)
    known = (b["kn"] & 1) == 1
    assert np.array_equal(fi[known, 0].view(np.uint64), b["fi0"][known, 0].view(np.uint64)), what + ": a known DOF was written"
    qc, qo = P.case_q(fi, b["truth_fi"], b["T"]["kappa"]).max(), P.case_q(b["oracle_fi"], b["truth_fi"], b["T"]["kappa"]).max()
    print("%-72s max q: gpu %.3g oracle %.3g" % (what, qc, qo))
    P.assert_parity(fi, b["oracle_fi"], b["truth_fi"], what)
    P.assert_per_case(fi, b["oracle_fi"], b["truth_fi"], b["T"]["kappa"], what)


@pytest.mark.parametrize("shape", tuple(SENS_KERNEL), ids=_ids)
def test_sensitivities_all_modes(wlsqm, oracle, shape):
    """`fit_many_device(..., sens=)`, dense rows, every family: the fast kernel the dispatch map names under (a) and (b), with the
    oracle's pattern of untouched and NaN entries; where the sensitivities come from the stored inverse (`sens-apply`) the fi of the same
    launch too, which is not the basic fit's kernel's.  Strict and accurate mode: the oracle's sensitivities bit for bit."""
    import wlsqm.hip as whip
    data = _shape_data(oracle, shape)
    for f in A.OP_FAMILIES:
        b = data[f]
        fi, sens, kern = _fit_with_sens(whip, b)
        assert kern == SENS_KERNEL[shape], (f, kern)
        _check_sens("sens fast [%s]" % kern, b, sens)
        if "truth_fi" in b:
            _check_fi("fi beside sens [%s]" % kern, b, fi)
        for mode in (True, "accurate"):
            fi, sens, kern = _fit_with_sens(whip, b, mode)
            assert kern == STRICT_SENS_KERNEL, (f, mode, kern)
            assert _same_bits(sens, b["oracle_sens"]), "sens, mode %s, %s %s: differs from the oracle" % (mode, f, shape)


@pytest.mark.parametrize("shape", STAGED_SHAPES, ids=_ids)
def test_sensitivities_on_the_staged_kernel(wlsqm, oracle, shape, monkeypatch):
    """The same under WLSQM_HIP_STAGE_SENS=a: one substitution per neighbour with the kept factor (csrc/fit_stage_iter.hip), no inverse."""
    import wlsqm.hip as whip
    data = _shape_data(oracle, shape)
    with monkeypatch.context() as env:
        env.setenv("WLSQM_HIP_STAGE_SENS", "a")
        for f in A.OP_FAMILIES:
            fi, sens, kern = _fit_with_sens(whip, data[f])
            assert kern == "stage-sens", (f, kern)
            _check_sens("sens fast [%s]" % kern, data[f], sens)


# ---- the adjoint of the fit ----------------------------------------------------------------------------------------------------------

def _check_gradients(route, b, field, gfk, gfi, scale=1.0):
    """grad_fk (n, K) and grad_fi (n, no) of g = scale * field `field` (scale a power of two times +-1: exact): the exact properties, then
    (a) and (b) for both gradients."""
    what, T = _what(route, b), b["T"]
    t_fk, t_fi, s = T["adjoint"][field]
    t_fk, t_fi, s = scale * t_fk, scale * t_fi, abs(scale) * s
    ref = b["ref"][field]
    rows = np.arange(b["K"])[None, :] < b["nk"][:, None]
    assert np.all(gfk[~rows] == 0.0), what + ": the padding of grad_fk is not exactly zero"
    assert np.all(gfi[T["kind"] == P.DOF_UNKNOWN] == 0.0), what + ": grad_fi of an unknown is not exactly zero"
    out = []
    for name, got, want, truth in (("grad_fk", gfk, scale * ref["grad_fk"], t_fk), ("grad_fi", gfi, scale * ref["grad_fi"], t_fi)):
        qc, qo = P.grad_q(got, truth, s, T["kappa"]), P.grad_q(want, truth, s, T["kappa"])
        out.append("%s gpu %.3g oracle %.3g" % (name, qc.max(), qo.max()))
        P.assert_scaled(P.grad_err(got, want, s), P.grad_err(got, truth, s), P.grad_err(want, truth, s), what + " " + name)
        P.assert_q(qc, qo, T["kappa"], what + " " + name)
    print("%-72s max q: %s" % (what, "  ".join(out)))


@pytest.mark.parametrize("shape", ADJOINT_SHAPES, ids=_ids)
def test_fit_adjoint_both_forms(wlsqm, oracle, shape, monkeypatch):
    """`fit_many_adjoint_device`, every family, the lane form and the rows form: both gradients under (a) and (b); the two forms agree
    bit for bit wherever tests/test_gpu_adjoint.py::test_both_forms demands it (everything but the 15-unknown system)."""
    import torch
    import wlsqm.hip as whip
    dim, order, K = shape
    data = _shape_data(oracle, shape)
    for f in A.OP_FAMILIES:
        b = data[f]
        got = {}
        for form, kernel in (("l", "adjoint-lane"), ("r", "adjoint-rows")):
            gfk, gfi = _full((N, K), float("nan")), _full((N, b["no"]), float("nan"))
            with monkeypatch.context() as env:
                env.setenv("WLSQM_HIP_ADJOINT_FORM", form)
                whip.fit_many_adjoint_device(dim, order, _t(b["xk"]), _t(b["nk"]), _t(b["xi"]), _t(b["kn"]), _t(b["wm"]), _t(b["g"][0]),
                                             grad_fk=gfk, grad_fi=gfi)
                ran = whip.last_kernel()
            torch.cuda.synchronize()
            assert ran == kernel, (f, form, ran)
            got[form] = (gfk.cpu().numpy(), gfi.cpu().numpy())
            _check_gradients("adjoint [%s]" % kernel, b, 0, *got[form])
        if b["no"] <= 10:
            assert _same_bits(got["l"][0], got["r"][0]) and _same_bits(got["l"][1], got["r"][1]), "%s %s: the two forms differ" % (f, shape)


@pytest.mark.parametrize("shape", CLOUD_SHAPES, ids=_ids)
def test_cloud_adjoint(wlsqm, oracle, shape):
    """`fit_cloud_adjoint_device`, index-based: a point table built from each family (A.point_table) and, for `lattice`, the real grid whose
    kNN rows start with the node itself.  The per-slot gradients and grad_fi under (a) and (b); grad_F is their scatter (on a point table
    every slot is a point of its own: the same bits)."""
    import torch
    import wlsqm.hip as whip
    dim, order, K = shape
    data = _shape_data(oracle, shape)
    for f in A.OP_FAMILIES:
        b = data[f]
        S, F, hoods, pidx = (b["S"], b["F"], b["hoods"], b["pidx"]) if f == "lattice" else A.point_table(b)
        slots, gfi = _full((N, K), float("nan")), _full((N, b["no"]), float("nan"))
        grad_F, _ = whip.fit_cloud_adjoint_device(dim, order, _t(S), _t(hoods), _t(b["nk"]), _t(b["kn"]), _t(b["wm"]), _t(b["g"][0]),
                                                  point_index=_t(pidx), grad_fi=gfi, slots=slots)
        torch.cuda.synchronize()
        assert whip.last_kernel() == "adjoint-lane", (f, whip.last_kernel())
        slots, gfi, grad_F = slots.cpu().numpy(), gfi.cpu().numpy(), grad_F.cpu().numpy()
        _check_gradients("index-based adjoint [adjoint-lane]", b, 0, slots, gfi)
        if f == "lattice":
            want, mag = np.zeros(len(F)), np.zeros(len(F))
            np.add.at(want, hoods.reshape(-1), slots.reshape(-1)); np.add.at(mag, hoods.reshape(-1), np.abs(slots.reshape(-1)))
            assert np.all(np.abs(grad_F - want) <= N * np.finfo(np.float64).eps * mag), f     # a node is in at most N rows
        else:
            assert _same_bits(grad_F[N:], slots.reshape(-1)) and np.all(grad_F[:N] == 0.0), f


# ---- the adjoint of the prepared solve -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SOLVE_SHAPES, ids=_ids)
def test_solve_adjoint(wlsqm, oracle, shape, monkeypatch):
    """`ExpertSolver.solve_many_adjoint_device` on a stack of three fields: g, -g / 2 (an exact scaling: its truth and its reference are
    those of the first field times -1/2) and another seed; through the stored operator's transpose on the matrix cores
    (WLSQM_HIP_SOLVE_ADJOINT=o) and through the geometric route (=g), each field against truth_adjoint_mp of its own g."""
    import torch
    import wlsqm.hip as whip
    dim, order, K = shape
    data = _shape_data(oracle, shape)
    for f in SOLVE_FAMILIES:
        b = data[f]
        s = wlsqm.ExpertSolver(dimension=dim, nk=b["nk"], order=b["order_a"], knowns=b["kn"], weighting_method=b["wm"],
                               algorithm=wlsqm.ALGO_BASIC, do_sens=False)
        s.prepare(xi=b["xi"], xk=b["xk"])
        g = _t(np.stack([b["g"][0], -0.5 * b["g"][0], b["g"][2]]))
        for switch, kernels in (("o", ("solve-op-adjoint-mfma",)), ("g", ("adjoint-rows", "adjoint-lane"))):
            gfk, gfi = _full((3, N, K), float("nan")), _full((3, N, b["no"]), float("nan"))
            with monkeypatch.context() as env:
                env.setenv("WLSQM_HIP_SOLVE_ADJOINT", switch)
                s.solve_many_adjoint_device(g, grad_fk=gfk, grad_fi=gfi)
                ran = whip.last_kernel()
            torch.cuda.synchronize()
            assert ran in kernels, (f, switch, ran)
            gfk, gfi = gfk.cpu().numpy(), gfi.cpu().numpy()
            for r, (field, scale) in enumerate(((0, 1.0), (0, -0.5), (2, 1.0))):
                _check_gradients("solve adjoint field %d [%s]" % (r, ran), b, field, gfk[r], gfi[r], scale)
        s.close()
