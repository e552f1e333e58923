"""CPU rehearsal of the adversarial families (tests/_adversarial.py) against the mpmath truth.

For every family and every shape the GPU tests use: the oracle is finite on every case (the inputs are ones the reference handles; no
case is dropped anywhere: the share of excluded cases is zero), and the CPU restatement of the fast kernels' arithmetic
(oracle/variants.c with the moment form, lane-split sums over 2 and 4 lanes, FMA contraction, the reciprocal in the weights and unscaled
LDL^T) as well as the accurate mode's (V_SYM) meet both criteria of tests/_parity.py against the oracle: the bar the GPU is held to is
reachable by its arithmetic before a GPU is involved.  Measured here (16 cases per family in four blocks of 4: centre / uniform weighting x
no knowns / F known, as A.combos draws them): the emulation's worst per-case q is between 0.2x and 2.6x the oracle's on every family and
shape, so Q_FLOOR = 0 suffices.  The real lattice with self-including rows (`lattice`) is rehearsed with the families.
"""
import numpy as np
import pytest

import _adversarial as A
import _parity as P

N_CASES = 16


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O


@pytest.mark.parametrize("dim,order,K", A.SHAPES)
def test_families_rehearsed_on_the_cpu(oracle, dim, order, K):
    fast = oracle.V_MOMENT | oracle.V_SPLIT | oracle.V_FMA | oracle.V_FASTW | oracle.V_LDLT
    n = N_CASES
    kn, wm = A.combos(n)
    excluded = 0
    for family in A.FAMILIES + ("lattice",):
        b = A.lattice_batch(dim, order, K, n) if family == "lattice" else A.make(family, dim, order, K, n)
        assert len(b["nk"]) == n                                                 # nothing filtered
        truth, kappa = A.truth_job((family, dim, order, K, n, 0, n))
        ora = b["fi0"].copy()
        oracle.fit_many(dim, b["xk"], b["fk"], b["nk"], b["xi"], ora, None, 0, b["order_a"], kn, wm)
        what = "%s %dD order %d K %d" % (family, dim, order, K)
        excluded += int((~np.isfinite(ora).all(axis=1)).sum())
        assert np.isfinite(ora).all(), what + ": the oracle is not finite"
        assert np.isfinite(kappa).all() and kappa.max() < 1e6, (what, kappa.max())
        for name, flags, nsplit in (("fast/2", fast, 2), ("fast/4", fast, 4), ("accurate", oracle.V_SYM, 1)):
            got = b["fi0"].copy()
            oracle.variant_fit_many(dim, order, b["xk"], b["fk"], b["nk"], b["xi"], got, kn, wm, flags=flags, nsplit=nsplit)
            P.assert_parity(got, ora, truth, what + " " + name)
            P.assert_per_case(got, ora, truth, kappa, what + " " + name)
            known = (kn & 1) == 1
            assert np.array_equal(got[known, 0], b["fi0"][known, 0]), what + ": known DOF changed"
    assert excluded == 0
