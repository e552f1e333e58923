"""GPU tests of the fit kernels on structured and adversarial neighbourhoods (tests/_adversarial.py): lattices with exact distance
ties (also at the largest distance), one-sided and stretched neighbourhoods, clouds far from the origin, kNN rows that contain the
point itself, data with a large offset or at the ends of the exponent range, exact polynomials.

Yardsticks (tests/_parity.py), both measured against the CPU oracle on the same inputs with the mpmath truth (`truth_fit_mp`):
  (a) per family batch, the standing column criterion  E_m <= 1e-10 + 8 N_m  (`assert_parity`);
  (b) per case,  max_j q_j(GPU) <= 8 max_j q_j(oracle) + Q_FLOOR  with q_j the case's error over eps kappa_j^2 (`assert_per_case`):
      one wrong lane cannot hide behind the worst-conditioned case of its batch.
Strict mode must equal the oracle bit for bit, accurate mode its CPU statement (oracle/variants.c with V_SYM) bit for bit.
Every family is a batch of 256 cases in four blocks of 64 (centre / uniform weighting x no knowns / function value known); the truths
of a shape are computed once per module, in worker processes that never touch the GPU.
"""
import numpy as np
import pytest

import _adversarial as A
import _parity as P
from _device_helpers import oracle, wlsqm  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

N = 256
SHAPES = A.SHAPES
SIDE_SHAPES = ((2, 2, 32), (2, 4, 64), (3, 2, 40), (1, 2, 8))          # the routes beside the dense one run these
STRICT_KERNELS = ("strict", "strict-rows", "strict-lane")
# the fast kernel family of a dense launch per shape (wlsqm.hip.last_kernel()): a quiet change of route is a failure
DENSE_KERNEL = {(2, 2, 32): "stage", (2, 3, 30): "stage", (2, 4, 64): "stage", (3, 2, 40): "stage", (3, 3, 64): "stage", (3, 4, 64): "quad",
                (1, 2, 8): "tile", (1, 4, 12): "tile"}
GATHER_KERNEL = {(2, 2, 32): "stage-gather", (2, 4, 64): "stage-gather", (3, 2, 40): "stage-gather", (1, 2, 8): "tile-gather"}
WORKERS = 12


def _t(a, dev="cuda:0"):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


_CACHE = {}


def _shape_data(oracle, shape):
    """All families of one shape (plus the real lattice with self-including rows): batch, knowns / weighting, the oracle's result, the
    mpmath truth and kappa.  Computed once per module."""
    if shape in _CACHE:
        return _CACHE[shape]
    dim, order, K = shape
    fams = A.FAMILIES + ("lattice",)
    step = 32
    jobs = [(f, dim, order, K, N, lo, lo + step) for f in fams for lo in range(0, N, step)]
    res = A.truths(jobs, WORKERS)
    out = {}
    kn, wm = A.combos(N)
    per = N // step
    for i, f in enumerate(fams):
        b = A.lattice_batch(dim, order, K, N) if f == "lattice" else A.make(f, dim, order, K, N)
        b["kn"], b["wm"] = kn, wm
        b["truth"] = np.concatenate([r[0] for r in res[i * per:(i + 1) * per]])
        b["kappa"] = np.concatenate([r[1] for r in res[i * per:(i + 1) * per]])
        ora = b["fi0"].copy()
        oracle.fit_many(dim, b["xk"], b["fk"], b["nk"], b["xi"], ora, None, 0, b["order_a"], kn, wm)
        assert np.isfinite(ora).all(), (f, shape)
        b["oracle"] = ora
        out[f] = b
    _CACHE[shape] = out
    return out


_OP_CACHE = {}


def _operator_truths(shape):
    """family -> truth of the fit's operator (A.operator_job, the operator alone: no adjoint is contracted) on the first A.N_OP cases of
    the family's batch of N, for the families of A.OP_FAMILIES: the operator does not see the data, and the data families (fk*, exactpoly*)
    are further draws of `plain`'s kind of geometry (every family seeds its own generator, so none of them IS plain's).  Once per module."""
    if shape not in _OP_CACHE:
        dim, order, K = shape
        step = 32
        per = A.N_OP // step
        fams = [f for f in A.FAMILIES if f in A.OP_FAMILIES]
        res = A.operators([(f, dim, order, K, N, lo, lo + step, ()) for f in fams for lo in range(0, A.N_OP, step)], WORKERS)
        _OP_CACHE[shape] = {f: A.operator_truth(f, dim, order, K, N, res[i * per:(i + 1) * per]) for i, f in enumerate(fams)}
    return _OP_CACHE[shape]


def _dense(whip, b, mode=None):
    import torch
    fi = _t(b["fi0"])
    with whip.strict(mode):
        whip.fit_many_device(b["dim"], b["order"], _t(b["xk"]), _t(b["fk"]), _t(b["nk"]), _t(b["xi"]), fi, _t(b["kn"]), _t(b["wm"]))
        torch.cuda.synchronize()
        kern = whip.last_kernel()
    return fi.cpu().numpy(), kern


def _check(route, b, got, ref=None):
    """Criteria (a) and (b) against the oracle, knowns bit-identical; prints max q (pytest -s shows the table of DESIGN section 2)."""
    ref = b["oracle"] if ref is None else ref
    what = "%s, %s %dD order %d K %d" % (route, b["family"], b["dim"], b["order"], b["K"])
    qc, qo = P.case_q(got, b["truth"], b["kappa"]).max(), P.case_q(ref, b["truth"], b["kappa"]).max()
    print("%-60s max q: gpu %.3g oracle %.3g" % (what, qc, qo))
    known = (b["kn"] & 1) == 1
    assert np.array_equal(_bits(got[known, 0]), _bits(b["fi0"][known, 0])), what + ": a known DOF was written"
    P.assert_parity(got, ref, b["truth"], what)
    P.assert_per_case(got, ref, b["truth"], b["kappa"], what)


def _accurate_expected(oracle, b):
    """Accurate mode: systems up to 10 unknowns in 2D / 3D carry the bits of variants.c V_SYM; 2D order 4, the larger 3D systems and 1D run
    the strict kernels (the oracle's bits)."""
    if b["dim"] == 1 or b["no"] > 10:
        return b["oracle"], STRICT_KERNELS
    sym = b["fi0"].copy()
    oracle.variant_fit_many(b["dim"], b["order"], b["xk"], b["fk"], b["nk"], b["xi"], sym, b["kn"], b["wm"], flags=oracle.V_SYM)
    return sym, ("accurate",)


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dD-o%d-K%d" % s)
def test_dense_fit_all_modes(wlsqm, oracle, shape):
    """`fit_many_device` on every family: the fast kernels under (a) and (b); strict mode bit-identical to the oracle; accurate mode
    bit-identical to its CPU statement — `tiny`, `huge` and `fkscale_*` are where its range checks must take the slow sequences."""
    import wlsqm.hip as whip
    data = _shape_data(oracle, shape)
    for f in A.FAMILIES + ("lattice",):
        b = data[f]
        got, kern = _dense(whip, b)
        assert kern in (DENSE_KERNEL[shape], DENSE_KERNEL[shape] + "-ragged"), (f, kern)
        _check("dense fast [%s]" % kern, b, got)
        got, kern = _dense(whip, b, True)
        assert kern in STRICT_KERNELS, (f, kern)
        bad = np.nonzero((_bits(got) != _bits(b["oracle"])).any(axis=1))[0]
        assert bad.size == 0, "strict mode, %s %s: cases %s differ from the oracle" % (f, shape, bad[:8])
        got, kern = _dense(whip, b, 2)
        want, kerns = _accurate_expected(oracle, b)
        assert kern in kerns, (f, kern)
        bad = np.nonzero((_bits(got) != _bits(want)).any(axis=1))[0]
        assert bad.size == 0, "accurate mode, %s %s: cases %s differ from the CPU statement (first: %r vs %r)" % (
            f, shape, bad[:8], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("shape", SIDE_SHAPES, ids=lambda s: "%dD-o%d-K%d" % s)
def test_index_based_fit(wlsqm, oracle, shape):
    """`fit_cloud_device`: a point table built from each family (origins, then every neighbour slot), and for the lattice a real grid
    whose kNN rows start with the node itself."""
    import torch
    import wlsqm.hip as whip
    dim, order, K = shape
    data = _shape_data(oracle, shape)
    for f in A.FAMILIES + ("lattice",):
        b = data[f]
        if f == "lattice":
            S, F, hoods, pidx = b["S"], b["F"], b["hoods"], b["pidx"]
        else:
            S, F, hoods, pidx = A.point_table(b)
        fi = _t(b["fi0"])
        whip.fit_cloud_device(dim, order, _t(S), _t(F), _t(hoods), fi, _t(b["nk"]), _t(b["kn"]), _t(b["wm"]), point_index=_t(pidx))
        torch.cuda.synchronize()
        kern = whip.last_kernel()
        assert kern == GATHER_KERNEL[shape], (f, kern)
        _check("index-based fast [%s]" % kern, b, fi.cpu().numpy())
        fi = _t(b["fi0"])
        whip.fit_cloud_device(dim, order, _t(S), _t(F), _t(hoods), fi, _t(b["nk"]), _t(b["kn"]), _t(b["wm"]), point_index=_t(pidx), strict=True)
        torch.cuda.synchronize()
        assert whip.last_kernel() in STRICT_KERNELS
        assert np.array_equal(_bits(fi.cpu().numpy()), _bits(b["oracle"])), "index-based strict, %s %s" % (f, shape)


@pytest.mark.parametrize("iterative", [False, True], ids=["basic", "iterative"])
@pytest.mark.parametrize("shape", SIDE_SHAPES, ids=lambda s: "%dD-o%d-K%d" % s)
def test_reference_signatures_with_sensitivities(wlsqm, oracle, shape, iterative):
    """`fit_*D_many_parallel(do_sens=1)` and `fit_*D_iterative_many_parallel` (numpy in / out): fi under (a) and (b) against the oracle's
    run of the same algorithm, sens against the oracle's under the column criterion, with a noise floor taken as the larger of the
    oracle's floor N_m of the fi column and eps kappa^2 of the batch's worst case — the forward error bound of a solve through the normal
    equations, which the sensitivities (columns of the inverse applied to unit data) see in full whereas a smooth field does not.  That
    bound is batch-wide: on the first A.N_OP cases of every family whose geometry differs (A.OP_FAMILIES) the basic fit's sens is also held to the per-case criterion (b)
    against the mpmath truth of the operator (`_parity.truth_operator_mp`), so that one wrong lane cannot hide behind the
    worst-conditioned case of its batch.  (The refinement's sensitivities are left at the column criterion.)"""
    import wlsqm.hip as whip
    dim, order, K = shape
    data = _shape_data(oracle, shape)
    name = "fit_%dD%s_many_parallel" % (dim, "_iterative" if iterative else "")
    kw = dict(max_iter=10) if iterative else {}
    for f in A.FAMILIES:
        b = data[f]
        no = b["no"]
        ref = b["fi0"].copy(); sens_o = np.full((N, K, no), 777.0)
        oracle.fit_many(dim, b["xk"], b["fk"], b["nk"], b["xi"], ref, sens_o, 1, b["order_a"], b["kn"], b["wm"], iterative=iterative, max_iter=10)
        fi = b["fi0"].copy(); sens = np.full((N, K, no), 777.0)
        getattr(wlsqm, name)(xk=b["xk"], fk=b["fk"], nk=b["nk"], xi=b["xi"], fi=fi, sens=sens, do_sens=1, order=b["order_a"], knowns=b["kn"],
                             weighting_method=b["wm"], **kw)
        kern = whip.last_kernel()
        assert kern and kern not in STRICT_KERNELS + ("accurate",), (f, kern)
        _check("%s [%s]" % (name, kern), b, fi, ref)
        live = np.arange(K)[None, :] < b["nk"][:, None]
        assert np.all(sens[~live] == 777.0), "%s %s: sens rows of unused slots were written" % (name, f)
        assert np.array_equal(np.isnan(sens), np.isnan(sens_o)), "%s %s: NaN pattern of sens" % (name, f)
        Nm = np.maximum(P.column_metric(ref, b["truth"]), np.finfo(np.float64).eps * b["kappa"].max() ** 2)
        E = P.column_metric(sens[live], sens_o[live])
        assert np.all(E <= P.TOL + P.NOISE_MULT * Nm), "%s %s: sens column metric %s, bound %s" % (name, f, E, P.TOL + P.NOISE_MULT * Nm)
        if not iterative and f in A.OP_FAMILIES:
            T = _operator_truths(shape)[f]
            m = A.N_OP
            assert np.array_equal(T["kappa"], b["kappa"][:m])
            qc, qo = (P.sens_q(x[:m], T["S"], T["live"], T["kappa"]) for x in (sens, sens_o))
            print("%-60s max q: gpu %.3g oracle %.3g" % ("%s sens [%s], %s" % (name, kern, f), qc.max(), qo.max()))
            P.assert_q(qc, qo, T["kappa"], "%s sens, %s %s" % (name, f, shape))


@pytest.mark.parametrize("shape", [(2, 2, 32), (3, 2, 40)], ids=lambda s: "%dD-o%d-K%d" % s)
def test_expert_solver_paths(wlsqm, oracle, shape, monkeypatch):
    """`ExpertSolver.prepare` + `solve`, and `solve_many_device` through the stored solution operator on the matrix cores, on the
    families whose geometry stresses the factorisation.  The second field of the stack is the first times -1/2 (known values too): an
    exact scaling of the whole problem, so its truth and its oracle result are those of the first times -1/2."""
    import torch
    import wlsqm.hip as whip
    dim, order, K = shape
    data = _shape_data(oracle, shape)
    monkeypatch.setenv("WLSQM_HIP_SOLVE_MANY", "op")
    for f in ("aniso", "far", "grid", "collinear"):
        b = data[f]
        s = wlsqm.ExpertSolver(dimension=dim, nk=b["nk"], order=b["order_a"], knowns=b["kn"], weighting_method=b["wm"],
                               algorithm=wlsqm.ALGO_BASIC, do_sens=False)
        s.prepare(xi=b["xi"], xk=b["xk"])
        fi = b["fi0"].copy()
        s.solve(fk=b["fk"], fi=fi)
        _check("ExpertSolver.solve [%s]" % whip.last_kernel(), b, fi)
        fks = np.stack([b["fk"], -0.5 * b["fk"]]); fi0 = np.stack([b["fi0"], -0.5 * b["fi0"]])
        got_d = _t(fi0)
        s.solve_many_device(_t(fks[:, :, :int(b["nk"].max())]), got_d)
        torch.cuda.synchronize()
        assert whip.last_kernel() == "solve-op-mfma", whip.last_kernel()
        got = got_d.cpu().numpy()
        _check("solve_many_device field 0 [solve-op-mfma]", b, got[0])
        half = dict(b, fi0=fi0[1], truth=-0.5 * b["truth"], oracle=-0.5 * b["oracle"])
        _check("solve_many_device field 1 [solve-op-mfma]", half, got[1])
        s.close()


@pytest.mark.parametrize("shape", [(2, 2, 32), (2, 4, 64), (3, 2, 40)], ids=lambda s: "%dD-o%d-K%d" % s)
@pytest.mark.parametrize("mode", [None, 2], ids=["fast", "accurate"])
def test_a_cases_bits_do_not_depend_on_the_families_in_its_batch(wlsqm, oracle, shape, mode):
    """One batch that interleaves all families (case i of the batch is case i // F of family i % F): every case comes out with the bits it
    has in its own family's batch.  The wave mates now include rows that defeat the sorted-neighbour guess of the staged kernel (shuffled
    lattice rows, ties at the largest distance, a self slot) beside rows that do not, and data 300 orders of magnitude apart."""
    import wlsqm.hip as whip
    data = _shape_data(oracle, shape)
    fams = A.FAMILIES + ("lattice",)
    own = {f: _dense(whip, data[f], mode)[0] for f in fams}
    F = len(fams)
    mixed = dict(data[fams[0]])
    for key in ("xk", "fk", "nk", "xi", "fi0", "kn", "wm"):
        mixed[key] = np.ascontiguousarray(np.stack([data[f][key] for f in fams], axis=1).reshape((N * F,) + data[fams[0]][key].shape[1:]))
    got, _ = _dense(whip, mixed, mode)
    got = got.reshape(N, F, -1)
    for i, f in enumerate(fams):
        bad = np.nonzero((_bits(got[:, i]) != _bits(own[f])).any(axis=1))[0]
        assert bad.size == 0, "%s %s: cases %s change their bits among other families" % (f, shape, bad[:8])


@pytest.mark.parametrize("shape", [(2, 2, 32), (2, 3, 30), (2, 4, 64), (3, 2, 40), (3, 3, 64)], ids=lambda s: "%dD-o%d-K%d" % s)
@pytest.mark.parametrize("route", ["dense", "index"])
def test_refuted_farthest_neighbour_guess(wlsqm, oracle, shape, route):
    """The staged kernel takes the last neighbour for the farthest when the last slots of EVERY row of a wave ascend, verifies the guess
    bit for bit and repeats the pass for the wave otherwise.  `sortedguess` and `grid_sorted` are whole waves of such rows (the two
    centre-weighted blocks of 64) in which some rows' farthest neighbour sits early in the row and others end on it (the lattice rows on a
    TIE at the largest distance): each case must come out with the bits it gets when the same batch is reversed row by row (descending
    rows: no wave speculates, the plain two passes), up to the change of summation order — so the comparison is (a) and (b) against the
    oracle on the forward batch (test_dense_fit_all_modes holds it for the dense route), and here: the cases whose guess is RIGHT and the
    cases whose guess is WRONG are held to the same per-case bound separately, so that a wave that skips the repeat (weights computed
    with too small a maximum in the refuted lanes only) cannot hide behind the others."""
    import torch
    import wlsqm.hip as whip
    dim, order, K = shape
    data = _shape_data(oracle, shape)
    for f in ("sortedguess", "grid_sorted"):
        b = data[f]
        if route == "dense":
            got, kern = _dense(whip, b)
        else:
            S, F, hoods, pidx = A.point_table(b)
            fi = _t(b["fi0"])
            whip.fit_cloud_device(dim, order, _t(S), _t(F), _t(hoods), fi, _t(b["nk"]), _t(b["kn"]), _t(b["wm"]), point_index=_t(pidx))
            torch.cuda.synchronize()
            got, kern = fi.cpu().numpy(), whip.last_kernel()
        assert kern.startswith("stage"), kern
        xk = b["xk"].reshape(N, K, -1); xi = b["xi"].reshape(N, -1)
        d2 = ((xk - xi[:, None, :]) ** 2).sum(axis=-1)
        d2 = np.where(np.arange(K)[None, :] < b["nk"][:, None], d2, -1.0)
        last = d2[np.arange(N), b["nk"] - 1]
        refuted = d2.max(axis=1) > last
        centre = b["wm"] == 2
        assert (refuted & centre).sum() >= 32 and (~refuted & centre).sum() >= 32
        for sel, name in ((refuted & centre, "refuted"), (~refuted & centre, "confirmed")):
            sub = dict(b, fi0=b["fi0"][sel], kn=b["kn"][sel], truth=b["truth"][sel], kappa=b["kappa"][sel], oracle=b["oracle"][sel])
            _check("%s staged fit, %s guesses" % (route, name), sub, got[sel])


@pytest.mark.parametrize("shape", [(2, 2, 32), (2, 3, 30), (2, 4, 64), (3, 2, 40), (3, 3, 64)], ids=lambda s: "%dD-o%d-K%d" % s)
def test_lattice_ties_at_the_largest_distance(wlsqm, oracle, shape):
    """Every case of `grid` has at least two neighbours at exactly the largest distance.  Strict mode exposes w: each of them has weight
    exactly 1e-4 (and no nearer neighbour has).  In every mode the sorted and the shuffled arrangement of the same neighbourhood (cases
    2i and 2i + 1) agree under the column criterion with the oracle's noise floor; that the fit itself is right is (a) and (b) of
    test_dense_fit_all_modes."""
    import torch
    import wlsqm.hip as whip
    dim, order, K = shape
    b = _shape_data(oracle, shape)["grid"]
    r2 = (b["lattice"]["steps"] ** 2).sum(axis=-1)
    valid = np.arange(K)[None, :] < b["nk"][:, None]
    far = valid & (r2 == np.where(valid, r2, 0).max(axis=1, keepdims=True))
    assert np.all(far.sum(axis=1) >= 2)
    fi = _t(b["fi0"])
    out = whip.strict_intermediates(dim, order, _t(b["xk"]), _t(b["fk"]), _t(b["nk"]), _t(b["xi"]), fi, _t(b["kn"]), _t(b["wm"]))
    torch.cuda.synchronize()
    w = out["w"].cpu().numpy()
    centre = b["wm"] == 2
    assert np.all(w[centre][far[centre]] == 1e-4), "a neighbour tied at the largest distance does not get weight exactly 1e-4"
    assert np.all(w[centre][(valid & ~far)[centre]] > 1e-4)
    Nm = P.column_metric(b["oracle"], b["truth"])
    for mode in (None, 2, True):
        got, _ = _dense(whip, b, mode)
        E = P.column_metric(got[1::2], got[0::2])
        assert np.all(E <= P.TOL + P.NOISE_MULT * Nm), "mode %s %s: sorted vs shuffled rows differ by %s (bound %s)" % (mode, shape, E, P.TOL + P.NOISE_MULT * Nm)
