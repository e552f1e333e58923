"""CPU rehearsal of the adversarial families (tests/_adversarial.py) against the mpmath truth.

For every family and every shape the GPU tests use: the oracle is finite on every case (the inputs are ones the reference handles; no
case is dropped anywhere: the share of excluded cases is zero), and the CPU restatement of the fast kernels' arithmetic
(oracle/variants.c with the moment form, lane-split sums over 2 and 4 lanes, FMA contraction, the reciprocal in the weights and unscaled
LDL^T) as well as the accurate mode's (V_SYM) meet both criteria of tests/_parity.py against the oracle: the bar the GPU is held to is
reachable by its arithmetic before a GPU is involved.  Measured here (16 cases per family in four blocks of 4: centre / uniform weighting x
no knowns / F known, as A.combos draws them): the emulation's worst per-case q is between 0.2x and 2.6x the oracle's on every family and
shape, so Q_FLOOR = 0 suffices.  The real lattice with self-including rows (`lattice`) is rehearsed with the families.

The fit's linear operator is rehearsed the same way (test_operator_families_rehearsed_on_the_cpu): on every family of A.OP_FAMILIES and every
shape the GPU tests of the sensitivities and the adjoints use, the oracle's sensitivities are finite on every live entry and they, and the
adjoint built from the oracle (tests/_adjoint_ref.py), stay a reference against the mpmath truths of tests/_parity.py.
"""
import numpy as np
import pytest

import _adversarial as A
import _parity as P

N_CASES = 16

# Shapes of the operator's GPU tests (tests/test_gpu_adversarial_operator.py): the sensitivities' and the adjoints' together.
OP_SHAPES = ((2, 2, 32), (2, 3, 30), (2, 4, 64), (3, 2, 40), (3, 3, 64), (1, 2, 8), (1, 4, 12))
# The oracle's worst per-case q over all of OP_SHAPES x A.OP_FAMILIES, 16 cases each, as measured by the test below (DESIGN section 2 has
# the whole table): sens 2.63 (grid, 3D order 3), grad_fk 2.79 (lattice, 1D order 2), grad_fi 15.8 (grid, 2D order 2; grad_fi is measured
# in the scale of grad_fk, and its one term per known is g itself).  Asserted: four times that, the margin for other seeds and another
# libm; beyond it the oracle has stopped being a reference for the quantity and the family's parameter has to move.
Q_ORACLE_MAX = {"sens": 2.63, "grad_fk": 2.79, "grad_fi": 15.8}
Q_MARGIN = 4.0


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


@pytest.mark.parametrize("dim,order,K", OP_SHAPES)
def test_operator_families_rehearsed_on_the_cpu(oracle, dim, order, K):
    """Sensitivities (do_sens=1) and the oracle-built adjoint against truth_operator_mp / truth_adjoint_mp: finite on every live entry,
    kappa below 1e6, and q within Q_MARGIN of the measured worst case.  No case is filtered."""
    import _adjoint_ref as R
    n = N_CASES
    for family in A.OP_FAMILIES:
        b = A.op_batch(family, dim, order, K, n)
        assert len(b["nk"]) == n
        T = A.operator_truth(family, dim, order, K, n)
        what = "%s %dD order %d K %d" % (family, dim, order, K)
        assert np.isfinite(T["kappa"]).all() and T["kappa"].max() < 1e6, (what, T["kappa"].max())
        sens = np.full((n, K, b["no"]), 777.0)
        fi = b["fi0"].copy()
        oracle.fit_many(dim, b["xk"], b["fk"], b["nk"], b["xi"], fi, sens, 1, b["order_a"], b["kn"], b["wm"])
        assert np.isfinite(sens[T["live"]]).all(), what + ": the oracle's sensitivities are not finite"
        rows = np.arange(K)[None, :] < b["nk"][:, None]
        known = ((b["kn"] & 1) == 1)[:, None] & rows
        assert np.all(sens[~rows] == 777.0) and np.isnan(sens[known][:, 0]).all(), what             # unused slots untouched; NaN marks the
        assert np.array_equal(np.isnan(sens), known[:, :, None] & (np.arange(b["no"]) == 0)), what    # known column and nothing else
        q = {"sens": P.sens_q(sens, T["S"], T["live"], T["kappa"]).max()}
        if R.covered(dim, order):
            g = A.op_g(family, dim, order, K, n, 0)
            ref = R.adjoint_ref(dim, order, b["xk"], b["nk"], b["xi"], b["kn"], b["wm"], g)
            t_fk, t_fi, s = T["adjoint"][0]
            assert np.isfinite(ref["grad_fk"]).all() and np.isfinite(ref["grad_fi"]).all(), what + ": the oracle-built adjoint is not finite"
            assert np.all(np.abs(ref["s"] - s) <= 1e-6 * s), what                                    # the same scale, from either side
            q["grad_fk"] = P.grad_q(ref["grad_fk"], t_fk, s, T["kappa"]).max()
            q["grad_fi"] = P.grad_q(ref["grad_fi"], t_fi, s, T["kappa"]).max()
        print("%-40s kappa %.3g  max q of the oracle: %s" % (what, T["kappa"].max(), "  ".join("%s %.3g" % kv for kv in q.items())))
        for name, v in q.items():
            assert v <= Q_MARGIN * Q_ORACLE_MAX[name], "%s: the oracle's %s is at q = %.3g: no reference" % (what, name, v)
