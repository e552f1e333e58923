"""Reference statements for the gradients through coupled solves (wlsqm.hip.differentiable_stencil_system_solve,
StencilSystemSolver.gradients, coupling_gradient and solve(transpose=True), csrc/krylov.hip's krylov_system_grads_kernel, DESIGN.md
section 25), numpy only, on tests/_krylov_system_ref.py, tests/_krylov_adjoint_ref.py and tests/_geometry_adjoint_ref.py.

M x = b with block (a, b) of M = D_ab + sum_o c[a, b, o] A_o, a loss L(x), g = dL/dx, M^T lam = g; all vectors (n, m).  Then
    dL/db = lam
    dL/dD_ab,i = -lam[i, a] x[i, b]
    dL/dc[a, b, o] = -sum_i lam[i, a] (A_o x[:, b])_i
    dL/dA_o[j, k] = -sum_b (sum_a c[a, b, o] lam[j, a]) x[k, b]                (per stored entry: a column named twice stays two entries)
and dL/dS at fixed neighbour lists is, summed over the components b, the geometry adjoint of the fit of F = x[:, b] (the F-known cases
given their own value) with g_j = -sum_o (sum_a c[a, b, o] lam[j, a]) rows[o] (rows[o, j] where the operator has per-case rows).
Block (a, b) of M^T is D_ba + sum_o c[b, a, o] A_o^T: the same kind of system on the transposed planes (transposed_system).

The order of operations of the gradient kernel, stated once (grads_statement), for row j with lam = lam[j]:
    once:  u[b][o] = c[0, b, o] * lam_0;  u[b][o] = fma(c[a, b, o], lam_a, u[b][o]) for a = 1 .. m - 1
    values (nop, total), per live entry e in entry order with column k, per plane o:
        t = u[0][o] * x[k, 0];  t = fma(u[b][o], x[k, b], t) for b = 1 .. m - 1;  values[o, soff[j // 64] + j % 64 + 64 e] = -t
    every padding position of every plane, the lanes of rows beyond n included: +0.0
    diag (m, m, n):  -(lam[j, a] * x[j, b]), one rounding

TRANSPOSED_CAPS[name] is the `maxiter` of the GPU tests' transposed solves: twice the count of _krylov_ref.bicgstab_ref on M^T (zero
start, rtol 1e-10, the right-hand side adjoint_rhs(n, m)) on the oracle's coefficients, which tests/test_krylov_system_adjoint_host.py
holds the constant to.  HOST_ONLY: the (name, preconditioner) whose count moves by 1.25x or more under the reversed summation order."""
from fractions import Fraction

import numpy as np

import _geometry_adjoint_ref as GA
import _krylov_system_ref as SR
import _stencil_ref as R
from _krylov_adjoint_ref import FD_BAR, central, entries_of, refined_loss  # noqa: F401 (the tests take them from here)

TRANSPOSED_CAPS = {
    "elasticity-2D-n130": {"jacobi": 70, None: 80},
    "elasticity-2D-n1000": {"jacobi": 378, None: 258},
    "elasticity-3D-n1000": {"jacobi": 62, None: 86},
    "reaction-2D-n130": {"jacobi": 18, None: 18},
    "random-m1": {"jacobi": 14, None: 34},
    "random-m2": {"jacobi": 28, None: 116},
    "random-m3": {"jacobi": 26, None: 152},
    "random-m4": {"jacobi": 28, None: 188},
}
HOST_ONLY = []
GPU_CASES = [(name, pc) for name, caps in TRANSPOSED_CAPS.items() for pc in caps if (name, pc) not in HOST_ONLY]
AUTOGRAD_SYSTEMS = ("elasticity-2D-n130", "reaction-2D-n130", "random-m3")


def adjoint_rhs(n, m):
    """(n, m): the right-hand side of the transposed solves, a loss's dL/dx (L = w . x has dL/dx = w)."""
    return np.random.default_rng([67, n, m]).standard_normal(n * m).reshape(n, m)


def transposed_diag(diag):
    """`diag` with (a, b) exchanged, in the form it came in."""
    d = np.asarray(diag, np.float64)
    return diag if d.ndim == 0 else np.ascontiguousarray(np.swapaxes(d, 0, 1))


def transposed_system(A, coupling, diag):
    """(A^T planes, coupling with (a, b) exchanged, diag with (a, b) exchanged): the system whose dense_matrix is M^T."""
    return (np.ascontiguousarray(np.transpose(A, (0, 2, 1))), np.ascontiguousarray(np.transpose(np.asarray(coupling, np.float64), (1, 0, 2))),
            transposed_diag(diag))


def transposed_structure(rows, n, nop):
    """(hoods, nk, slots (nop, n, K)) of the operator packed from the transposed rows (no own entries): R.transpose_rows' order, which is
    the order of StencilOperator.prepare_transpose."""
    trows = R.transpose_rows(rows, n)
    K = max(1, max(len(r) for r in trows))
    hoods, nk, slots = np.zeros((n, K), np.int32), np.zeros(n, np.int32), np.full((nop, n, K), np.nan)
    for i, r in enumerate(trows):
        nk[i] = len(r)
        for e, (col, v) in enumerate(r):
            hoods[i, e], slots[:, i, e] = col, v
    return hoods, nk, slots


def grads_statement(sell, n, coupling, lam, x, check=None):
    """(at, values (nop, len(at)), diag (m, m, len(check))) in the stated order of operations, every fma rounded once: the positions of
    the live entries of the rows `check` (default: all) in (row, entry) order, the kernel's bits there, and its diag on those rows."""
    coupling = np.asarray(coupling, np.float64)
    m, nop = coupling.shape[0], coupling.shape[2]
    check = np.arange(n) if check is None else np.asarray(check)
    ln, soff, col = np.asarray(sell["len"], np.int64), np.asarray(sell["soff"], np.int64), np.asarray(sell["col"])
    at, vals = [], []
    diag = np.zeros((m, m, len(check)))
    for k, j in enumerate(check):
        u = np.zeros((m, nop))
        for b in range(m):
            for o in range(nop):
                t = coupling[0, b, o] * lam[j, 0]
                for a in range(1, m):
                    t = SR.fma(coupling[a, b, o], lam[j, a], t)
                u[b, o] = t
        for e in range(int(ln[j])):
            p = int(soff[j // 64] + j % 64 + 64 * e)
            c = int(col[p])
            v = np.zeros(nop)
            for o in range(nop):
                t = u[0, o] * x[c, 0]
                for b in range(1, m):
                    t = SR.fma(u[b, o], x[c, b], t)
                v[o] = -t
            at.append(p)
            vals.append(v)
        diag[:, :, k] = -(lam[j][:, None] * x[j][None, :])
    return np.array(at, np.int64), (np.array(vals).T if at else np.zeros((nop, 0))), diag


def exact_values(sell, n, coupling, lam, x, check=None):
    """(exact, mag) (nop, entries): -sum_ab c[a, b, o] lam[j, a] x[k, b] of every live entry of the rows `check` in exact arithmetic,
    rounded once, and the sum of the magnitudes of its m^2 terms."""
    coupling = np.asarray(coupling, np.float64)
    m, nop = coupling.shape[0], coupling.shape[2]
    check = np.arange(n) if check is None else np.asarray(check)
    ln, soff, col = np.asarray(sell["len"], np.int64), np.asarray(sell["soff"], np.int64), np.asarray(sell["col"])
    F = lambda v: Fraction(float(v))
    exact, mag = [], []
    for j in check:
        for e in range(int(ln[j])):
            c = int(col[int(soff[j // 64] + j % 64 + 64 * e)])
            ex, mg = np.zeros(nop), np.zeros(nop)
            for o in range(nop):
                terms = [F(coupling[a, b, o]) * F(lam[j, a]) * F(x[c, b]) for a in range(m) for b in range(m)]
                ex[o], mg[o] = float(-sum(terms, Fraction(0))), float(sum((abs(t) for t in terms), Fraction(0)))
            exact.append(ex)
            mag.append(mg)
    return np.array(exact).T, np.array(mag).T


def implicit_gradients(A, coupling, diag, b, g):
    """dict(x, lam (n, m), b, diag (m, m, n), coupling (m, m, nop), entries (nop, n, n): dL/dA_o[j, k]) by dense solves."""
    coupling = np.asarray(coupling, np.float64)
    n, m = b.shape
    M = SR.dense_matrix(A, coupling, diag)
    x = np.linalg.solve(M, b.reshape(-1)).reshape(n, m)
    lam = np.linalg.solve(M.T, g.reshape(-1)).reshape(n, m)
    return dict(x=x, lam=lam, b=lam, diag=-np.einsum("ia,ib->abi", lam, x), coupling=-np.einsum("ia,oij,jb->abo", lam, A, x),
                entries=-np.einsum("abo,ja,kb->ojk", coupling, lam, x))


def geometry_truth(sy, x, lam, coupling=None):
    """dL/dS (n, dim) of a fit system at fixed x, lam (n, m) and neighbour lists: per component b GA.geometry_adjoint_ref on the fit of
    F = x[:, b] with g_j = -sum_o (sum_a c[a, b, o] lam[j, a]) rows[o], its per-slot gradients scattered to the neighbours and the
    own-point rows to the points; the m results summed."""
    coupling = np.asarray(sy["coupling"] if coupling is None else coupling, np.float64)
    n, dim, S, hoods, m = sy["n"], sy["dim"], sy["S"], sy["hoods"], sy["m"]
    rows = sy["rows"]                                            # (nop, no) or (nop, n, no)
    no = rows.shape[-1]
    per_case = np.broadcast_to(rows if rows.ndim == 3 else rows[:, None, :], (rows.shape[0], n, no))
    T = np.zeros_like(S)
    for b in range(m):
        u = lam @ coupling[:, b, :]                              # (n, nop)
        g = np.ascontiguousarray(-np.einsum("jo,ojn->jn", u, per_case))
        fi_in = np.zeros((n, no))
        fi_in[:, 0] = x[:, b]
        xb = np.ascontiguousarray(x[:, b])
        ref = GA.geometry_adjoint_ref(dim, sy["order"], np.ascontiguousarray(S[hoods]), np.ascontiguousarray(xb[hoods]), sy["nk"], S, fi_in,
                                      sy["knowns"], sy["wm"], g)
        part = np.zeros_like(S)
        np.add.at(part, hoods.reshape(-1), ref["grad_xk"].reshape(-1, dim))
        T += part + ref["grad_xi"]
    return T
