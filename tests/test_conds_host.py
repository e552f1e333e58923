"""CPU side of the condition-number tests (tests/_conds_ref.py): the committed truths are what mpmath gives today, the fp64 statement of
the kernel and LAPACK both sit within a few units of eps kappa^2 of them, and the families are what tests/test_gpu_conds.py takes them
for — so that the GPU test cannot hide behind a condition nobody checked.  No device."""
import numpy as np
import pytest

import _cases as K
import _conds_ref as R
import _parity as P

# The two cases of sweep_1d.npz beyond KAPPA_MAX (order 3 and 4 with a mask that leaves 4 unknowns on nk = 4 neighbours: interpolation, not
# a fit).  The golden is taken as it is, so they stay, are held to the same bound in units of eps kappa^2, and are named here; at
# kappa eps ~ 1e-7 they are nowhere near the no-digits class.
MIXED_1_STEEP = {53: 5.1e8, 99: 2.9e8}


def _nr(f):
    return np.array([R._nr(f["dim"], f["order"][j], f["knowns"][j]) for j in range(len(f["nk"]))])


def test_fixture_holds_todays_truth():
    """Every 8th case of every family, recomputed in mpmath, equals the fixture to 1e-25 relative; the digest of the inputs matches."""
    from mpmath import mp, mpf
    checked = 0
    for name in R.names():
        f = R.family(name)
        hi, lo = R.truth(name)                                   # checks the digest
        cases = list(range(0, len(f["nk"]), 8))
        again = R.truth_mp(*R.args(f), cases=cases)
        with mp.workdps(R.DPS):
            for j, k in zip(cases, again):
                if k is None:
                    assert np.isnan(hi[j]), (name, j)
                elif np.isinf(R.split(k)[0]):
                    assert np.isinf(hi[j]), (name, j)
                else:
                    assert abs(mpf(float(hi[j])) + mpf(float(lo[j])) - k) <= mpf(1e-25) * k, (name, j)
                checked += 1
    assert checked >= 300


def test_statement_and_lapack_sit_on_the_truth():
    """q = |x - truth| / (eps truth^2) of the fp64 statement and of the reference (LAPACK on the statement's scaled matrix; for the sweep
    goldens the reference's own A and scales), per family.  Q_REF is held from both sides, and the statement, the CPU stand-in of the
    kernel, passes the bound of the GPU test."""
    worst_ref, worst_st = 0.0, 0.0
    for name in R.names():
        f = R.family(name)
        T = R.truth(name)[0]
        reg = R.regular(name)
        st = R.statement(*R.args(f))
        ref = R.sweep_reference(f["dim"]) if name.startswith("mixed") else R.reference(*R.args(f))
        assert np.array_equal(np.isnan(st), np.isnan(T)) and np.array_equal(np.isnan(ref), np.isnan(T)), name
        q_st, q_ref = R.q_units(st[reg], T[reg]), R.q_units(ref[reg], T[reg])
        print("%-12s %3d regular cases, kappa <= %.3g: q_statement %.3f  q_reference %.3f" % (name, reg.sum(), T[reg].max(), q_st.max(), q_ref.max()))
        worst_ref, worst_st = max(worst_ref, float(q_ref.max())), max(worst_st, float(q_st.max()))
        deg = f["degenerate"]
        assert (~np.isfinite(st[deg]) | (st[deg] >= R.HUGE)).all(), name
    print("largest q_reference %.3f (Q_REF %.3g), largest q_statement %.3f (GPU bound %.3g)"
          % (worst_ref, R.Q_REF, worst_st, P.NOISE_MULT * max(1.0, R.Q_REF)))
    assert R.Q_REF / 4 <= worst_ref <= R.Q_REF, "set Q_REF to %.1f" % (np.ceil(11.5 * worst_ref) / 10)
    assert worst_st <= P.NOISE_MULT * max(1.0, R.Q_REF)


def test_families_are_what_the_gpu_test_takes_them_for():
    ran = set()
    for name in R.names():
        f = R.family(name)
        T = R.truth(name)[0]
        nr, deg, n = _nr(f), f["degenerate"], len(f["nk"])
        # nr < 1 gives no value, and only that
        assert np.array_equal(np.isnan(T), nr < 1), name
        # the no-digits class is the degenerate family's marked cases, nothing else; nobody else is excluded
        with np.errstate(invalid="ignore"):
            no_digits = np.isinf(T) | (T * R.EPS >= R.NO_DIGITS)
        assert np.array_equal(no_digits, deg), (name, np.flatnonzero(no_digits != deg))
        assert deg.any() == (name == "degenerate")
        assert np.array_equal(R.regular(name), (nr >= 1) & ~deg)
        steep = np.flatnonzero(R.regular(name) & (np.nan_to_num(T) > R.KAPPA_MAX))
        if name == "mixed_1":
            assert sorted(steep) == sorted(MIXED_1_STEEP) and all(T[j] <= MIXED_1_STEEP[j] for j in steep)
        else:
            assert len(steep) == 0, (name, steep, T[steep])
        # nr == 1: the statement gives exactly 1.0
        one = np.flatnonzero((nr == 1) & ~deg)
        st = R.statement(*R.args(f, one))
        assert (st == 1.0).all() and (T[one] == 1.0).all(), name
        if name.startswith("uniform"):
            dim, order = int(name.split("_")[1]), int(name.split("_")[2])
            no = K.NDOF[dim][order]
            ran.add((dim, order))
            assert n == (66 if no >= 20 else 130) and n % 64 == 2 and (f["order"] == order).all()
            assert f["xk"].shape[1] == 2 * no + 4 and f["nk"][0] == 2 * no + 4 and len(set(f["nk"].tolist())) > 1
            assert (f["nk"] >= np.minimum(nr + 2, 2 * no + 4)).all()
            for kind in range(6):                               # every kind of mask under both weightings
                sel = np.arange(n) % 6 == kind
                assert set(f["wm"][sel].tolist()) == {1, 2} and all(f["knowns"][j] == R.mask(kind, no, j) for j in np.flatnonzero(sel))
            for sel in (nr == 1, nr < 1):                       # at least three times each, in different blocks
                where = np.flatnonzero(sel)
                assert len(where) >= 3 and len(set((where // 64).tolist())) >= 2, name
            if no >= 4:
                assert any(len(P._unknown_set(dim, order, int(kn))[3]) == 2 for kn in f["knowns"])      # stray bits drop unknowns
        if name.startswith("mixed") or name == "chunks":
            assert set(f["order"].tolist()) == {0, 1, 2, 3, 4}                  # the order_arr route: five launches on one workspace
            assert set(f["wm"].tolist()) == {1, 2} and len(set(f["knowns"].tolist())) > 4
        if name == "chunks":
            assert f["dim"] == 1 and f["xk"].shape == (130, 8)
        if name == "degenerate":
            assert n == 130 and deg.sum() >= 30 and (f["order"] == 2).all() and f["dim"] == 2
            short = deg & (f["nk"] < nr)
            assert short.sum() >= 8 and (f["nk"][short] == nr[short] - 1).all()
    assert ran == set(R.DIMS_ORDERS)


def test_balanced_family_sees_a_coarser_rotation_threshold():
    """Columns orthogonal but for rho in 1e-13 .. 1e-7: the statement with the kernel's threshold is on the truth (measured above), the
    same statement with 1e-9 skips the one rotation where rho is below it and is wrong by 2 rho, far outside the GPU bound."""
    f = R.family("balanced")
    T = R.truth("balanced")[0]
    assert ((T - 1.0 > 1e-14) & (T - 1.0 < 1e-6)).all(), (T.min() - 1.0, T.max() - 1.0)
    q = R.q_units(R.statement(*R.args(f), jacobi_tol=1e-9), T)
    print("balanced: %d of %d cases beyond the bound with a rotation threshold of 1e-9, the worst at %.3g units" % ((q > 16).sum(), len(q), q.max()))
    assert (q > 1e3 * P.NOISE_MULT * max(1.0, R.Q_REF)).sum() >= 16
