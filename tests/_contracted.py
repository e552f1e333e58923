"""What the CPU and the GPU tests of the CONTRACTED numerics mode share: the mode's CPU statement (oracle/variants.c with
V_SYM | V_FMA: the accurate mode's arithmetic with a += b * c fused in the neighbour sums, the LU update and the substitutions) and the
criteria of the sweep goldens."""
import numpy as np

import _cases as K
import _parity as P

TOL = 1e-10                # north star: relative, per column — asserted as it stands, no spare factor (config_C5_16M is at 9.0e-11)


def flags(oracle):
    return oracle.V_SYM | oracle.V_FMA


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def taken(dim, order):
    """Shapes the accurate kernels (and so their fused instantiations) take: the 2D / 3D systems up to 10 unknowns."""
    return dim in (2, 3) and K.NDOF[dim][order] <= 10


def statement(oracle, dim, order, xk, fk, nk, xi, fi0, kn, wm, fl=None):
    """One uniform-order batch through variants.c with the mode's flags (any flags with `fl`)."""
    out = np.ascontiguousarray(np.array(fi0, np.float64, copy=True))
    c = np.ascontiguousarray
    oracle.variant_fit_many(dim, order, c(xk), c(fk), c(nk), c(xi), out, c(kn), c(wm), flags=flags(oracle) if fl is None else fl)
    return out


def expected(oracle, dim, order, xk, fk, nk, xi, fi0, kn, wm):
    """What a contracted-mode call must return: the CPU statement on the shapes the kernels take — every case, whatever its mask —
    and the oracle (the strict kernels) on every other shape."""
    if taken(dim, order):
        return statement(oracle, dim, order, xk, fk, nk, xi, fi0, kn, wm)
    ora = np.array(fi0, np.float64, copy=True)
    oracle.fit_many(dim, xk, fk, nk, xi, ora, None, 0, np.full(len(nk), order, np.int32), kn, wm, ntasks=8)
    return ora


def differing_cases(got, want):
    """Indices of the cases whose rows differ: the NaN patterns must coincide and every other double must have the same bits (the
    payload of a NaN is the one thing an x86 host and the GPU do not share)."""
    got = np.asarray(got, np.float64); want = np.asarray(want, np.float64)
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    bad = (nan_g != nan_w) | ((bits(got) != bits(want)) & ~nan_w)
    return np.nonzero(bad.reshape(len(got), -1).any(axis=1))[0]


def sweep_top(dim):
    return 3 if dim == 2 else 2


def sweep_statement(oracle, dim):
    """The sweep golden of `dim` through the CPU statement, order by order (variants.c takes one order per call).  Returns (contracted
    result, oracle result, extended-precision truth, the golden dict); the orders the kernels do not take are the oracle's."""
    d = K.sweep(dim)
    ora = d["fi_in"].copy()
    oracle.fit_many(dim, d["xk"], d["fk"], d["nk"], d["xi"], ora, None, 0, d["order"], d["knowns"], d["wm"], ntasks=8)
    got = ora.copy()
    for o in range(sweep_top(dim) + 1):
        sel = np.nonzero(d["order"] == o)[0]
        no = K.NDOF[dim][o]
        got[sel, :no] = statement(oracle, dim, o, d["xk"][sel], d["fk"][sel], d["nk"][sel], d["xi"][sel], d["fi_in"][sel][:, :no],
                                  d["knowns"][sel], d["wm"][sel])
    truth = P.truth_fit(dim, d["xk"], d["fk"], d["nk"], d["xi"], d["fi_in"], d["order"], d["knowns"], d["wm"])
    return got, ora, truth, d


def check_sweep(got, ora, truth, d, dim, what):
    """Per order of the sweep golden: P.assert_parity against the REFERENCE's fi (1e-10 + 8 N with N the reference's own distance from
    the extended-precision solution), and no further from that solution than twice the oracle's distance plus 1e-12.  Prints the
    figures; returns the worst Ea / (2 Es + 1e-12)."""
    worst = 0.0
    for o in range(sweep_top(dim) + 1):
        sel = d["order"] == o
        no = K.NDOF[dim][o]
        P.assert_parity(got[sel, :no], d["fi"][sel, :no], truth[sel, :no], "%s, sweep dim %d order %d" % (what, dim, o))
        Ea = P.column_metric(got[sel, :no], truth[sel, :no]); Es = P.column_metric(ora[sel, :no], truth[sel, :no])
        r = float(np.max(Ea / (2.0 * Es + 1e-12)))
        worst = max(worst, r)
        print("%s, sweep dim %d order %d: Ea %.3e  Es %.3e  Ea / (2 Es + 1e-12) = %.2f" % (what, dim, o, Ea.max(), Es.max(), r))
        assert np.all(Ea <= 2.0 * Es + 1e-12), (dim, o, Ea, Es)
    return worst
