"""ExpertSolver(debug=True).conds() on the GPU (csrc/conds.hip, wlsqm_hip_expert_conds) against the mpmath truth of
tests/_conds_ref.py, on the families described there: every (dimension, order) instantiation of the kernel, the per-case order route,
the chunk loop, ragged nk, both weightings, masks of every kind, degenerate neighbourhoods beside regular ones, and nearly orthogonal
columns at the edge of the Jacobi rotation test.

Bound of a regular case: |got - truth| <= NOISE_MULT * max(1, Q_REF) * eps * truth^2 — the project's multiplier over what LAPACK on the
same fp64 matrix is measured to need (tests/test_conds_host.py), since the kernel's one-sided Jacobi and a bidiagonal SVD are different
algorithms.  nr < 1 gives NaN and nr == 1 gives 1.0, both exactly.  A degenerate case has no digits to hold: its value is non-finite or at
least 2^40.  Every test prints the largest observed ratio before it asserts."""
import numpy as np
import pytest

import _conds_ref as R
import _parity as P

pytestmark = pytest.mark.gpu

BOUND = P.NOISE_MULT * max(1.0, R.Q_REF)
# family, cases taken (None: all), and the kernel instantiation a uniform-order batch runs (None: the per-case order route)
TABLE = ([("uniform_%d_%d" % do, None, do) for do in R.DIMS_ORDERS]
         + [("uniform_2_2", 1, (2, 2)), ("uniform_2_2", 64, (2, 2))]          # one lane alone; one full block alone
         + [("mixed_%d" % d, None, None) for d in (1, 2, 3)] + [("chunks", None, None), ("degenerate", None, (2, 2)), ("balanced", None, (1, 1))])


@pytest.fixture(scope="module")
def wlsqm():
    import wlsqm as W
    from wlsqm import _binding
    assert _binding.lib().wlsqm_hip_device_count() >= 1, "no HIP device: the GPU tests need a real MI355X"
    return W


def _solver(W, f, sel=slice(None), debug=True, host=None, prepare=True):
    s = W.ExpertSolver(dimension=f["dim"], nk=f["nk"][sel], order=f["order"][sel], knowns=f["knowns"][sel],
                       weighting_method=f["wm"][sel], debug=debug, host=host)
    if prepare:
        s.prepare(xi=np.ascontiguousarray(f["xi"][sel]), xk=np.ascontiguousarray(f["xk"][sel]))
    return s


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _hold(what, got, f, T, sel=slice(None)):
    """The assertions on one batch's values against the truths T of the same cases; returns the largest ratio to the bound's unit."""
    nr = np.array([R._nr(f["dim"], o, kn) for o, kn in zip(f["order"][sel], f["knowns"][sel])])
    deg = f["degenerate"][sel]
    assert got.shape == nr.shape
    assert np.array_equal(np.isnan(got), nr < 1), (what, np.flatnonzero(np.isnan(got) != (nr < 1))[:8])
    one = (nr == 1) & ~deg
    assert (got[one] == 1.0).all(), (what, got[one][got[one] != 1.0][:8])
    reg = (nr >= 1) & ~deg
    q = R.q_units(got[reg], T[reg])
    print("%s: %d regular cases, kappa <= %.3g, largest |got - truth| / (eps truth^2) = %.3f (bound %g)"
          % (what, reg.sum(), T[reg].max(), q.max(), BOUND))
    j = int(np.argmax(q))
    assert q.max() <= BOUND, (what, int(np.flatnonzero(reg)[j]), got[reg][j], T[reg][j])
    if deg.any():
        print("%s: degenerate cases give %s ..." % (what, got[deg][:6]))
        assert (~np.isfinite(got[deg]) | (got[deg] >= R.HUGE)).all(), (what, got[deg])
    return float(q.max())


def test_table_reaches_every_instantiation():
    """All 15 cond_kernel<DIM, ORDER> run from a uniform-order batch (order_arr == nullptr), and the per-case order route runs in every
    dimension."""
    assert {t[2] for t in TABLE if t[2] is not None} == set(R.DIMS_ORDERS)
    for name, _, inst in TABLE:
        f = R.family(name)
        if inst is not None:
            assert f["dim"] == inst[0] and (f["order"] == inst[1]).all()
        else:
            assert set(f["order"].tolist()) == {0, 1, 2, 3, 4}
    assert {R.family(t[0])["dim"] for t in TABLE if t[2] is None} == {1, 2, 3}


@pytest.mark.parametrize("name,head", [t[:2] for t in TABLE if t[0] != "chunks"], ids=["%s%s" % (t[0], "" if t[1] is None else "_head%d" % t[1])
                                                                                        for t in TABLE if t[0] != "chunks"])
def test_family_against_truth(wlsqm, name, head):
    f = R.family(name)
    sel = slice(None) if head is None else slice(0, head)
    T = R.truth(name)[0][sel]
    s = _solver(wlsqm, f, sel)
    got = s.conds()
    _hold(name, got, f, T, sel)
    if name.startswith("mixed"):                                # and to the reference's own figure, at the bound plus its own share
        ref = R.sweep_reference(f["dim"])
        reg = R.regular(name)
        q = R.q_units(got[reg], ref[reg])
        print("%s: largest |got - reference| / (eps reference^2) = %.3f" % (name, q.max()))
        assert q.max() <= BOUND + R.Q_REF
    assert np.array_equal(_bits(s.conds()), _bits(got))           # a second call: the same bits
    guest = _solver(wlsqm, f, sel, host=s)                        # a guest shares the geometry: the same bits
    assert np.array_equal(_bits(guest.conds()), _bits(got))
    guest.close(); s.close()


def test_two_chunks_of_mixed_orders(wlsqm):
    """n = 32768 + 130 cases, the 130 of `chunks` repeated with period 130: the second chunk of wlsqm_hip_expert_conds (case0 = 32768)
    starts at case 8 of the period.  One lane per case and no cross-lane step: the bits are a function of the case."""
    base = R.family("chunks")
    n = 32768 + 130
    idx = np.arange(n) % 130
    f = dict(dim=1, xi=base["xi"][idx], xk=base["xk"][idx], nk=base["nk"][idx], order=base["order"][idx], knowns=base["knowns"][idx],
             wm=base["wm"][idx], degenerate=base["degenerate"][idx])
    s = _solver(wlsqm, f)
    got = s.conds()
    s.close()
    assert got.shape == (n,)
    print("cases 32764 .. 32771 (period cases %s): %s" % (idx[32764:32772].tolist(), got[32764:32772]))
    _hold("chunks", got[:130], base, R.truth("chunks")[0])
    differ = np.flatnonzero(_bits(got) != _bits(got[:130])[idx])
    assert len(differ) == 0, (len(differ), differ[:8], got[differ[:8]], got[idx[differ[:8]]])


def test_conds_needs_prepare_and_debug(wlsqm):
    f = R.family("uniform_2_2")
    s = _solver(wlsqm, f, prepare=False)
    with pytest.raises(RuntimeError):
        s.conds()                                                # not prepared yet
    s2 = _solver(wlsqm, f, debug=False)
    with pytest.raises(RuntimeError):
        s2.conds()                                               # not in debug mode
