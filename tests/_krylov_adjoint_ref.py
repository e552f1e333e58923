"""Reference statements for the gradients through implicit solves (wlsqm.hip.differentiable_stencil_solve, StencilSolver.gradients,
csrc/krylov.hip's krylov_grads_kernel), numpy only, on tests/_krylov_ref.py and tests/_geometry_adjoint_ref.py.

M(theta) x = b, a loss L(x), g = dL/dx, M^T lam = g.  With M = diag(d) + c A:
    dL/db = lam,   dL/dd_i = -lam_i x_i,   dL/dc = -(lam, A x),   dL/dA[j, k] = -c lam_j x_k,
and dL/dS at fixed neighbour lists is the geometry adjoint of the fit of F = x (the F-known cases given their own value) with
g_j = -c lam_j rows[o]: row j of A applied to x is rows[o] . fi_out[j] of that fit.

The constants: TRANSPOSED_COUNTS are the iteration counts of KR.bicgstab_ref on M^T (Jacobi, zero start, rtol 1e-10, the right-hand side
adjoint_rhs(n)) on the CPU oracle's coefficients, measured when this file was written, in the order of KR.SYSTEMS; the GPU tests' cap is
twice the count, as section 17 does for the forward solves, and tests/test_krylov_adjoint_host.py holds the constants to a fresh run."""
import numpy as np

import _geometry_adjoint_ref as GA
import _krylov_ref as KR
import _stencil_ref as R

TRANSPOSED_COUNTS = dict(zip(KR.SYSTEMS, (14, 8, 279, 61, 22, 59, 20, 15, 7, 8)))
FD_BAR = 1e-7               # formula against central differences, relative, at the better of h = 1e-5 and 1e-6


def transposed_maxiter(name):
    return 2 * TRANSPOSED_COUNTS[name]


def adjoint_rhs(n):
    """The right-hand side of the transposed solves: a loss's dL/dx."""
    return np.random.default_rng([31, n]).standard_normal(n)


def implicit_gradients(A, d, c, b, g):
    """dict(x, lam, b, diag, scale, entries (n, n): dL/dA[j, k]) by dense solves."""
    M = np.diag(d) + c * A
    x = np.linalg.solve(M, b)
    lam = np.linalg.solve(M.T, g)
    return dict(x=x, lam=lam, b=lam, diag=-lam * x, scale=-float(lam @ (A @ x)), entries=-c * np.outer(lam, x))


def diag_vector(sy):
    return np.asarray(sy["diag"], np.float64) if np.ndim(sy["diag"]) else np.full(sy["n"], float(sy["diag"]))


def operator_dense(sy, S=None):
    """A of a fit system with the points at S (default: where the system has them), from the CPU oracle's coefficients."""
    moved = sy if S is None else dict(sy, S=S)
    return (KR.dense_of(moved) - np.diag(diag_vector(sy))) / sy["scale"]


def geometry_truth(sy, x, lam):
    """dL/dS (n, dim) of a fit system at fixed x, lam and neighbour lists: GA.geometry_adjoint_ref on the fit of F = x with
    g_j = -c lam_j rows[o], its per-slot gradients scattered to the neighbours and the own-point rows to the points."""
    n, dim, S, hoods = sy["n"], sy["dim"], sy["S"], sy["hoods"]
    rows = sy["rows"][0]                                         # (no,) or (n, no)
    no = rows.shape[-1]
    g = np.ascontiguousarray((-sy["scale"] * lam)[:, None] * np.broadcast_to(rows, (n, no)))
    fi_in = np.zeros((n, no))
    fi_in[:, 0] = x
    ref = GA.geometry_adjoint_ref(dim, sy["order"], np.ascontiguousarray(S[hoods]), np.ascontiguousarray(x[hoods]), sy["nk"], S, fi_in,
                                  sy["knowns"], sy["wm"], g)
    T = np.zeros_like(S)
    np.add.at(T, hoods.reshape(-1), ref["grad_xk"].reshape(-1, dim))
    return T + ref["grad_xi"]


def refined_loss(w, M, b, steps=3):
    """w . x of M x = b in extended precision (numpy's longdouble): a LAPACK solve refined on residuals formed in longdouble, so that a
    central difference of it is limited by its step, not by the rounding of the fp64 solve (for a derivative of 1e-4 of L's size and
    h = 1e-6, eps |L| / (2 h |dL|) is 1e-6 in fp64: more than FD_BAR)."""
    ld = np.longdouble
    Ml, bl = M.astype(ld), b.astype(ld)
    x = np.linalg.solve(M, b).astype(ld)
    for _ in range(steps):
        x = x + np.linalg.solve(M, (bl - Ml @ x).astype(np.float64)).astype(ld)
    return w.astype(ld) @ x


def central(f, h):
    return float((f(h) - f(-h)) / (2.0 * h))


def entries_of(m, nrows):
    """(row, position) of every live entry of a SELL-64 matrix m = dict(len, soff, ...), in (row, entry) order."""
    ln = np.asarray(m["len"], np.int64)[:nrows]
    row = np.repeat(np.arange(nrows), ln)
    e = np.arange(len(row)) - np.repeat(np.cumsum(ln) - ln, ln)
    return row, np.asarray(m["soff"], np.int64)[row // 64] + 64 * e + row % 64


def grads_statement(m, nrows, c, lam, x):
    """(values (total,), diag (nrows,)) as krylov_grads_kernel states them, two roundings each product: -((c lam_j) x_col) at the live
    entries and +0.0 elsewhere; -(lam_j x_j)."""
    row, at = entries_of(m, nrows)
    values = np.zeros(int(np.asarray(m["soff"])[-1]))
    values[at] = -((c * lam[row]) * x[np.asarray(m["col"])[at]])
    return values, -(lam * x)


def exact_triple(a, b, c):
    """(sum a_i b_i c_i, sum |a_i b_i c_i|) of three finite float arrays as Fractions, in integer arithmetic: KR.exact_dot with a third
    factor."""
    from fractions import Fraction
    parts = [np.frexp(np.ravel(np.asarray(v, np.float64))) for v in (a, b, c)]
    ints = [np.ldexp(mant, 53).astype(np.int64).tolist() for mant, _ in parts]
    e = sum(ex.astype(np.int64) for _, ex in parts) - 159
    e = e.tolist()
    emin = min(e) if e else 0
    total = mag = 0
    for p, q, r, k in zip(ints[0], ints[1], ints[2], e):
        t = (p * q * r) << (k - emin)
        total += t
        mag += abs(t)
    two = Fraction(2) ** emin
    return total * two, mag * two
