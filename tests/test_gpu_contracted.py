"""GPU tests of the CONTRACTED numerics mode (mode 3; csrc/fit_accurate.hip with FMA = true): the accurate mode with a += b * c fused
in the neighbour sums of the matrix and of the right-hand side, in the LU update and in the two substitutions.  Checker: oracle/variants.c
with V_SYM | V_FMA (tests/_contracted.py) — every case the accurate kernels take must equal it BIT FOR BIT on every path (speculative
single pass, two-pass repeat, clean-up kernel, per-lane rows), every other case the oracle (the strict kernels).  Against the reference's
own output (tests/golden/config_*_1M.npz, config_C5_16M.npz) every column must be within 1e-10 — the bound as it stands: the CPU
statement is at 9.0e-11 on config_C5_16M (tests/test_contracted_cpu.py).  Mirrors tests/test_gpu_accurate.py."""
import numpy as np
import pytest

import _adversarial as A
import _cases as K
import _contracted as CT
import _parity as P

pytestmark = pytest.mark.gpu

TOL = CT.TOL
KERNEL = "accurate-fma"
STRICT_KERNELS = ("strict", "strict-rows", "strict-lane")


@pytest.fixture(scope="module")
def wlsqm():
    import wlsqm as W
    from wlsqm import _binding
    assert _binding.lib().wlsqm_hip_device_count() >= 1, "no HIP device: the GPU tests need a real MI355X"
    return W


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O


def _t(a, dev="cuda:0"):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _fit(whip, dim, order, xk, fk, nk, xi, fi0, kn, wm, mode=3):
    """One dense device-resident call in `mode`: (result, kernel family)."""
    import torch
    fi = _t(fi0)
    with whip.strict(mode):
        whip.fit_many_device(dim, order, _t(xk), _t(fk), _t(nk), _t(xi), fi, _t(kn), _t(wm))
        torch.cuda.synchronize()
        kern = whip.last_kernel()
    return fi.cpu().numpy(), kern


def _same(got, want, what):
    bad = CT.differing_cases(got, want)
    assert bad.size == 0, "%s: cases %s differ from the CPU statement (first: %r vs %r)" % (what, bad[:8], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("name", K.DENSE)
def test_contracted_mode_at_the_headline_density(wlsqm, oracle, name):
    """BASELINE configs[1] / configs[4] at the density the metric is quoted on: bit-identical to variants.c V_SYM | V_FMA, the fused kernels
    ran, E_m <= 1e-10 on EVERY column against the reference's own output — and NOT the accurate mode's bits.  configs[2] (14 unknowns) runs
    the strict arithmetic as in the accurate mode: the oracle's bits."""
    import wlsqm.hip as whip
    c = K.config_dense(name)
    dim, order, no = c["dim"], c["order"], c["no"]
    args = (dim, order, c["xk"], c["fk"], c["nk_a"], c["xi"], c["fi0"], c["knowns_a"], c["wm_a"])
    got, kern = _fit(whip, *args)
    want = CT.expected(oracle, *args)
    _same(got, want, name)
    if no <= 10:
        assert kern == KERNEL, kern
        E = P.column_metric(got, c["g"]["fi"])
        print("%s: contracted mode vs the reference, E_max %.3e" % (name, E.max()))
        assert np.all(E <= TOL), "%s: E = %s" % (name, E)
        acc, kern2 = _fit(whip, *args, mode=2)
        assert kern2 == "accurate", kern2
        differ = (CT.bits(got) != CT.bits(acc)).any(axis=1)
        print("%s: %d of %d cases differ in bits from the accurate mode" % (name, differ.sum(), len(differ)))
        assert differ.any(), "%s: the contracted mode returned the accurate mode's bits" % name
        assert np.array_equal(CT.bits(acc), CT.bits(CT.statement(oracle, *args, fl=oracle.V_SYM))), "the accurate mode changed"
    else:
        assert kern == "strict-rows", kern


def test_contracted_mode_with_the_default_mask(wlsqm, oracle):
    """knowns = b?_F, the default of every fit_* function: the fused kernels take the cases, bit-identical to the CPU statement (the
    elimination of impl.pyx:792-823 stays term by term, unfused), the known column is not written, and every derivative column is within
    1e-10 of the ORACLE's."""
    import wlsqm.hip as whip
    for name in ("C2_1M", "C5_1M", "C5_16M"):
        c = K.config_dense(name)
        dim, order = c["dim"], c["order"]
        n = len(c["nk_a"])
        kn = np.ones(n, np.int64)
        args = (dim, order, c["xk"], c["fk"], c["nk_a"], c["xi"], c["fi0"], kn, c["wm_a"])
        got, kern = _fit(whip, *args)
        assert kern == KERNEL, kern
        _same(got, CT.expected(oracle, *args), name)
        assert np.array_equal(CT.bits(got[:, 0]), CT.bits(c["fi0"][:, 0])), "the known value is not written"
        ora = c["fi0"].copy()
        oracle.fit_many(dim, c["xk"], c["fk"], c["nk_a"], c["xi"], ora, None, 0, np.full(n, order, np.int32), kn, c["wm_a"], ntasks=8)
        E = P.column_metric(got[:, 1:], ora[:, 1:])
        print("%s, F known: contracted mode vs the oracle, E_max %.3e" % (name, E.max()))
        assert np.all(E <= TOL), "%s: E = %s" % (name, E)


def _hetero(dim, order, Kn, n, seed, wlsqm):
    """The batches of tests/test_gpu_accurate.py (same generator, same seeds)."""
    rng = np.random.default_rng(seed)
    no = K.NDOF[dim][order]
    xi = rng.uniform(0, 1, (n, dim))
    xk = xi[:, None, :] + 0.05 * rng.uniform(-1, 1, (n, Kn, dim))
    fk = np.sin(3 * xk[..., 0]) * np.cos(2 * xk[..., -1])
    nk = rng.integers(min(Kn, no + 3), Kn + 1, n).astype(np.int32); nk[::5] = Kn
    masks = [0, 0, 0, 1, 1, 2, 5, (1 << (no - 1)) | 2, (1 << no) - 1, 1 << (no + 1), (1 << (no + 2)) | 1] if no > 2 else [0, 0, 1]
    kn = rng.choice(np.array(masks, np.int64), n)
    wm = rng.choice(np.array([wlsqm.WEIGHT_UNIFORM, wlsqm.WEIGHT_CENTER], np.int32), n)
    fi0 = rng.uniform(-1, 1, (n, no)); fi0[:, 0] = np.sin(3 * xi[:, 0]) * np.cos(2 * xi[:, -1])
    return dict(xi=xi, xk=xk, fk=fk, nk=nk, kn=kn, wm=wm, fi0=fi0, no=no)


def _args(b, dim, order):
    return (dim, order, b["xk"], b["fk"], b["nk"], b["xi"], b["fi0"], b["kn"], b["wm"])


@pytest.mark.parametrize("dim,order,Kn", [(2, 0, 8), (2, 1, 12), (2, 2, 32), (2, 2, 30), (2, 2, 18), (2, 3, 40), (3, 0, 6), (3, 1, 14),
                                          (3, 2, 40), (3, 2, 26), (2, 2, 7), (3, 2, 33), (2, 4, 64), (2, 4, 40), (2, 4, 37)])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_contracted_mode_heterogeneous_batches(wlsqm, oracle, dim, order, Kn, n):
    """Ragged nk, both weightings, knowns masks (none / F / one derivative / two / everything / stray high bits), batch sizes around the
    64-case groups, odd K (per-lane rows instead of the LDS staging): every case carries the bits of the CPU statement (2D order 4: the
    oracle's — the strict kernels) — per CASE, whatever shares its group."""
    import wlsqm.hip as whip
    b = _hetero(dim, order, Kn, n, 7 * Kn + n, wlsqm)
    got, kern = _fit(whip, *_args(b, dim, order))
    assert kern == ("strict-rows" if (dim, order) == (2, 4) else KERNEL), kern
    bad = CT.differing_cases(got, CT.expected(oracle, *_args(b, dim, order)))
    assert bad.size == 0, "cases %s (knowns %s, nk %s)" % (bad[:8], b["kn"][bad[:8]], b["nk"][bad[:8]])


def test_contracted_mode_is_layout_and_tile_mate_independent(wlsqm, oracle):
    """The same cases as contiguous rows (LDS staging), as strided device views and index-based (per-lane rows), permuted, and through a
    per-case order tensor (order buckets: case_index): the same bits per case."""
    import torch
    import synth
    import wlsqm.hip as whip
    rng = np.random.default_rng(5)
    npts, n, Kn = 5000, 1500, 32
    S = synth.halton(npts, 2); F = synth.field(S)
    pidx = rng.permutation(npts)[:n].astype(np.int32)
    hoods = synth.knn(S, Kn, query=pidx).astype(np.int32)
    nk = rng.integers(10, Kn + 1, n).astype(np.int32); nk[::4] = Kn
    kn = rng.choice(np.array([0, 0, 0, 1, 4], np.int64), n)
    wm = rng.choice(np.array([wlsqm.WEIGHT_UNIFORM, wlsqm.WEIGHT_CENTER], np.int32), n)
    hc = np.where(np.arange(Kn)[None, :] < nk[:, None], hoods, 0).astype(np.int64)
    xk, fk, xi = S[hc], F[hc], S[pidx]
    fi0 = rng.uniform(-1, 1, (n, 6)); fi0[:, 0] = F[pidx]
    want = CT.expected(oracle, 2, 2, xk, fk, nk, xi, fi0, kn, wm)
    with whip.contracted():
        fi = _t(fi0)
        whip.fit_many_device(2, 2, _t(xk), _t(fk), _t(nk), _t(xi), fi, _t(kn), _t(wm))
        torch.cuda.synchronize()
        assert whip.last_kernel() == KERNEL
        _same(fi.cpu().numpy(), want, "dense")
        # strided device views: every second slot of a wider array
        xw = torch.zeros((n, 2 * Kn, 2), dtype=torch.float64, device="cuda:0"); xw[:, ::2] = _t(xk)
        fw = torch.zeros((n, 2 * Kn), dtype=torch.float64, device="cuda:0"); fw[:, ::2] = _t(fk)
        fi = _t(fi0)
        whip.fit_many_device(2, 2, xw[:, ::2], fw[:, ::2], _t(nk), _t(xi), fi, _t(kn), _t(wm))
        torch.cuda.synchronize()
        assert whip.last_kernel() == KERNEL
        _same(fi.cpu().numpy(), want, "strided")
        # index-based
        hp = hoods.copy(); hp[np.arange(Kn)[None, :] >= nk[:, None]] = -1
        fi = _t(fi0)
        whip.fit_cloud_device(2, 2, _t(S), _t(F), _t(hp), fi, _t(nk), _t(kn), _t(wm), point_index=_t(pidx))
        torch.cuda.synchronize()
        assert whip.last_kernel() == KERNEL
        _same(fi.cpu().numpy(), want, "index-based")
        # ... and with the mode given per call
    fi = _t(fi0)
    whip.fit_cloud_device(2, 2, _t(S), _t(F), _t(hp), fi, _t(nk), _t(kn), _t(wm), point_index=_t(pidx), strict="contracted")
    torch.cuda.synchronize()
    assert whip.last_kernel() == KERNEL and whip.get_strict() is False
    _same(fi.cpu().numpy(), want, "index-based, strict='contracted'")
    with whip.contracted():
        # permuted: a case's bits do not depend on its neighbours in the batch
        perm = rng.permutation(n)
        fi = _t(fi0[perm])
        whip.fit_many_device(2, 2, _t(xk[perm]), _t(fk[perm]), _t(nk[perm]), _t(xi[perm]), fi, _t(kn[perm]), _t(wm[perm]))
        torch.cuda.synchronize()
        _same(fi.cpu().numpy(), want[perm], "permuted")
        # order buckets (case_index) of a per-case order tensor: the order-2 cases keep their bits
        orders = rng.choice(np.array([1, 2], np.int32), n)
        fi = _t(fi0)
        whip.fit_many_device(2, _t(orders), _t(xk), _t(fk), _t(nk), _t(xi), fi, _t(kn), _t(wm), max_order=2)
        torch.cuda.synchronize()
        sel = orders == 2
        _same(fi.cpu().numpy()[sel], want[sel], "order buckets")


def test_contracted_mode_outside_the_safe_range_of_its_fast_sequences(wlsqm, oracle):
    """Operands the speculative pass cannot vouch for send the group to the clean-up kernel (the IEEE sequences): coordinates scaled by
    1e-40 / 1e+40 and 1e-120 / 1e+120, a neighbour AT the centre, an empty neighbourhood, a NaN coordinate and a NaN value, every neighbour
    at the centre — bit-identical to the CPU statement, NaN patterns included; cases that share a wave with them too."""
    import wlsqm.hip as whip
    n, Kn = 256, 32
    b = _hetero(2, 2, Kn, n, 3, wlsqm)
    b["kn"][:] = 0
    scale = np.ones(n); scale[10:20] = 1e-40; scale[70:75] = 1e40; scale[130] = 1e-120; scale[131] = 1e120
    b["xk"] = b["xk"] * scale[:, None, None]; b["xi"] = b["xi"] * scale[:, None]
    b["xk"][200, 3] = b["xi"][200]                       # a neighbour at the centre
    b["nk"][201] = 0                                      # nothing to fit: the reference divides 0 by 0
    b["xk"][202, 5, 1] = np.nan
    b["fk"][203, 7] = np.nan
    b["xk"][204, :, :] = b["xi"][204]                     # every neighbour at the centre: max_d2 = 0
    for full in (False, True):                            # ragged rows (two-pass form), then full rows (speculative pass + clean-up kernel)
        if full:
            b["nk"][:] = Kn; b["nk"][201] = 0
        got, kern = _fit(whip, *_args(b, 2, 2))
        assert kern == KERNEL, kern
        with np.errstate(all="ignore"):
            want = CT.expected(oracle, *_args(b, 2, 2))
        assert np.isnan(want).any() and not np.isnan(want[:10]).any()
        _same(got, want, "full rows" if full else "ragged rows")


def test_contracted_mode_on_unsorted_rows(wlsqm, oracle):
    """Rows in no order refute the farthest-neighbour guess of the speculative pass: the wave repeats the sums on the spot with the true
    maximum (the two-pass repeat).  Whole batches of shuffled rows, full (nk == K, K a multiple of the chunk), in 2D and 3D."""
    import wlsqm.hip as whip
    for dim, order, Kn, n in ((2, 2, 32, 1000), (3, 2, 40, 640), (2, 3, 40, 320)):
        b = _hetero(dim, order, Kn, n, 17 + Kn, wlsqm)
        b["nk"][:] = Kn
        rng = np.random.default_rng(Kn)
        for j in range(n):
            perm = rng.permutation(Kn)
            b["xk"][j] = b["xk"][j][perm]; b["fk"][j] = b["fk"][j][perm]
        got, kern = _fit(whip, *_args(b, dim, order))
        assert kern == KERNEL, kern
        _same(got, CT.expected(oracle, *_args(b, dim, order)), "shuffled rows, %dD order %d" % (dim, order))


def test_contracted_mode_through_the_reference_signatures_and_expertsolver(wlsqm, oracle):
    """The mode is a property of the calling thread: fit_2D_many_parallel, fit_3D_many and ExpertSolver.solve on host arrays take it too."""
    import wlsqm.hip as whip
    b = _hetero(2, 2, 32, 777, 99, wlsqm)
    orders = np.full(777, 2, np.int32)
    want = CT.expected(oracle, *_args(b, 2, 2))
    b3 = _hetero(3, 2, 40, 333, 98, wlsqm)
    want3 = CT.expected(oracle, *_args(b3, 3, 2))
    with whip.contracted():
        fi = b["fi0"].copy()
        wlsqm.fit_2D_many_parallel(b["xk"], b["fk"], b["nk"], b["xi"], fi, None, 0, orders, b["kn"], b["wm"], ntasks=8)
        assert whip.last_kernel() == KERNEL
        _same(fi, want, "fit_2D_many_parallel")
        fi = b3["fi0"].copy()
        wlsqm.fit_3D_many(b3["xk"], b3["fk"], b3["nk"], b3["xi"], fi, None, 0, np.full(333, 2, np.int32), b3["kn"], b3["wm"])
        assert whip.last_kernel() == KERNEL
        _same(fi, want3, "fit_3D_many")
        es = wlsqm.ExpertSolver(dimension=2, nk=b["nk"], order=orders, knowns=b["kn"], weighting_method=b["wm"],
                                algorithm=wlsqm.ALGO_BASIC, do_sens=False)
        es.prepare(xi=b["xi"], xk=b["xk"])
        fi = b["fi0"].copy()
        es.solve(fk=b["fk"], fi=fi)
        es.close()
        assert whip.last_kernel() == KERNEL
        _same(fi, want, "ExpertSolver.solve")
        # sensitivities and refinement are the strict kernels', as in the accurate mode
        fi = b["fi0"].copy(); sens = np.zeros((777, 32, 6))
        wlsqm.fit_2D_many_parallel(b["xk"], b["fk"], b["nk"], b["xi"], fi, sens, 1, orders, b["kn"], b["wm"], ntasks=8)
        assert whip.last_kernel() in STRICT_KERNELS, whip.last_kernel()


def test_contracted_mode_across_streams_graphs_and_repeated_calls(wlsqm, oracle):
    """Many calls in a row on one stream, calls alternating between two streams, batches whose groups DO take the two-pass repeat (unsorted
    neighbours) and cases with stray mask bits, and a call captured into a HIP graph and replayed must all return the bits of a fresh call."""
    import torch
    import wlsqm.hip as whip
    rng = np.random.default_rng(21)
    b = _hetero(2, 2, 32, 1000, 5, wlsqm)
    b["nk"][:] = 32
    for j in range(0, 1000, 3):                                   # a third of the cases with shuffled neighbours: their groups are redone
        perm = rng.permutation(32)
        b["xk"][j] = b["xk"][j][perm]; b["fk"][j] = b["fk"][j][perm]
    want = CT.expected(oracle, *_args(b, 2, 2))
    args = [_t(b[k]) for k in ("xk", "fk", "nk", "xi")]
    kn, wm = _t(b["kn"]), _t(b["wm"])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with whip.contracted():
        outs = []
        for rep in range(7):                                       # one stream, back to back; then alternating streams
            for st in ((None,) if rep < 3 else (s1, s2)):
                fi = _t(b["fi0"])
                if st is None:
                    whip.fit_many_device(2, 2, *args, fi, kn, wm)
                else:
                    st.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(st):
                        whip.fit_many_device(2, 2, *args, fi, kn, wm)
                outs.append(fi)
        torch.cuda.synchronize()
        for fi in outs:
            _same(fi.cpu().numpy(), want, "repeated calls")
        # captured and replayed
        fi = _t(b["fi0"])
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s1):
            whip.fit_many_device(2, 2, *args, fi, kn, wm)
        for rep in range(3):
            fi.copy_(_t(b["fi0"]))
            g.replay()
            torch.cuda.synchronize()
            _same(fi.cpu().numpy(), want, "replay %d" % rep)
        fi2 = _t(b["fi0"])                                          # and an eager call on the captured stream afterwards
        with torch.cuda.stream(s1):
            whip.fit_many_device(2, 2, *args, fi2, kn, wm)
        torch.cuda.synchronize()
        _same(fi2.cpu().numpy(), want, "eager call after the capture")


# ---- the families of tests/_adversarial.py -------------------------------------------------------------------------------------------

N_ADV = 256
FAMS = A.FAMILIES + ("lattice",)
_ADV = {}


def _family(shape, f):
    if (shape, f) not in _ADV:
        dim, order, Kn = shape
        b = A.lattice_batch(dim, order, Kn, N_ADV) if f == "lattice" else A.make(f, dim, order, Kn, N_ADV)
        b["kn"], b["wm"] = A.combos(N_ADV)
        _ADV[(shape, f)] = b
    return _ADV[(shape, f)]


@pytest.mark.parametrize("shape", A.SHAPES, ids=lambda s: "%dD-o%d-K%d" % s)
def test_contracted_mode_on_the_adversarial_families(wlsqm, oracle, shape):
    """Lattices with exact distance ties, one-sided and stretched neighbourhoods, clouds far from the origin, rows that contain the point
    itself, data with a large offset or at the ends of the exponent range, exact polynomials (256 cases per family: centre / uniform
    weighting x no knowns / F known): at the shapes the kernels take, bit for bit the CPU statement — `tiny`, `huge`, the `_edge` and the
    `fkscale_*` families are where the range checks must hand the group to the IEEE sequences; at every other shape the oracle's bits."""
    import wlsqm.hip as whip
    dim, order, Kn = shape
    for f in FAMS:
        b = _family(shape, f)
        got, kern = _fit(whip, *_args(b, dim, order))
        assert (kern == KERNEL) if CT.taken(dim, order) else (kern in STRICT_KERNELS), (f, kern)
        with np.errstate(all="ignore"):
            want = CT.expected(oracle, *_args(b, dim, order))
        _same(got, want, "%s %s" % (f, shape))


@pytest.mark.parametrize("shape", [(2, 2, 32), (2, 3, 30), (3, 2, 40)], ids=lambda s: "%dD-o%d-K%d" % s)
def test_a_cases_bits_do_not_depend_on_the_families_in_its_batch(wlsqm, oracle, shape):
    """One batch that interleaves all families (case i of the batch is case i // F of family i % F): every case comes out with the bits it
    has in its own family's batch — and those are the CPU statement's."""
    import wlsqm.hip as whip
    dim, order, Kn = shape
    own = {f: _fit(whip, *_args(_family(shape, f), dim, order))[0] for f in FAMS}
    F = len(FAMS)
    mixed = {}
    for key in ("xk", "fk", "nk", "xi", "fi0", "kn", "wm"):
        first = _family(shape, FAMS[0])[key]
        mixed[key] = np.ascontiguousarray(np.stack([_family(shape, f)[key] for f in FAMS], axis=1).reshape((N_ADV * F,) + first.shape[1:]))
    got, kern = _fit(whip, *_args(mixed, dim, order))
    assert kern == KERNEL, kern
    got = got.reshape(N_ADV, F, -1)
    for i, f in enumerate(FAMS):
        bad = CT.differing_cases(got[:, i], own[f])
        assert bad.size == 0, "%s %s: cases %s change their bits among other families" % (f, shape, bad[:8])
    with np.errstate(all="ignore"):
        _same(got.reshape(N_ADV * F, -1), CT.expected(oracle, *_args(mixed, dim, order)), "interleaved %s" % (shape,))


@pytest.mark.parametrize("dim", [2, 3])
def test_contracted_mode_vs_the_reference_sweep_goldens(wlsqm, oracle, dim):
    """The mode against the REFERENCE's own output on tests/golden/sweep_{2,3}d.npz through the host path (every order, both weightings, a
    sweep of knowns masks incl. stray bits, ragged nk), with the criteria of the CPU test (tests/_contracted.py: check_sweep), and bit for
    bit the CPU statement; the orders the strict kernels take carry the strict mode's bits."""
    import wlsqm.hip as whip
    want, ora, truth, d = CT.sweep_statement(oracle, dim)
    many = getattr(wlsqm, "fit_%dD_many_parallel" % dim)
    fi = d["fi_in"].copy()
    with whip.contracted():
        rc = many(xk=d["xk"], fk=d["fk"], nk=d["nk"], xi=d["xi"], fi=fi, sens=None, do_sens=0, order=d["order"], knowns=d["knowns"],
                  weighting_method=d["wm"], ntasks=8)
    assert rc == 0
    CT.check_sweep(fi, ora, truth, d, dim, "contracted mode")
    _same(fi, want, "sweep dim %d" % dim)
