"""Reference statements for the sparse approximate inverse preconditioner (wlsqm.hip.ApproximateInverse, csrc/krylov.hip's
krylov_spai_kernel), numpy only.

M = diag(d) + c A as per-row lists, `M_rows[r] = (d_r, [(column, c * value), ...])` in entry order (m_rows makes them from
tests/_stencil_ref.rows_of's).  An own entry (column r in row r) is part of the diagonal: a row is read as d_r plus its own entries in entry
order, then its other entries.  Row i of Q has one unknown per slot: slot 0 the diagonal (column i), slot k the stored entry k - 1.  A slot
whose column an earlier slot names is dead: coefficient 0.0.  With J the columns of the live slots, the rows M[J, :] as a dense block B
over the columns that they name:

  lstsq statement:  q = argmin ||B^T q - e_i||_2                                  (numpy.linalg.lstsq)
  Gram statement:   G = B B^T, rhs = B[:, i], G q = rhs by L D L^T without pivoting, in the kernel's order of summation:
                    B[b] sums the entries of row J[b] that name one column in entry order, the diagonal first;
                    G[a, b], b <= a, is the sum over the entries of row J[a] AS STORED, the diagonal first, of entry * B[b, its column];
                    the factorisation is right-looking, step k taking l = G[k + 1:, k] / G[k, k] off the trailing rows.
                    (The kernel fuses each multiply-add; numpy rounds twice.)

CAPS[name][method] is the `maxiter` of the GPU solves: twice the iteration count of tests/_krylov_block_ref.bicgstab_block_ref /
tests/_krylov_l2_ref.bicgstab2_ref on that system with the lstsq statement's Q as the preconditioner (zero start, rtol 1e-10), which
tests/test_krylov_spai_host.py measures on the oracle's coefficients and holds the constants to."""
import numpy as np

import _krylov_l2_ref as L2
import _krylov_ref as KR
import _stencil_ref as R

EPS = 2.0 ** -53
METHODS = ("bicgstab2", "bicgstab")


def system(name):
    """tests/_krylov_l2_ref.system: the systems of tests/_krylov_ref.py on clouds in Morton order, and the 3D ones at tau 1."""
    return L2.system(name)


def rows_of_system(sy, slots=None, own=None):
    """tests/_stencil_ref.rows_of for the system `sy`: from the given coefficients (the GPU tests pass the operator's own), from the random
    structure, or for a fit from the CPU oracle's (tests/_krylov_ref.dense_of's)."""
    if sy["kind"] == "random":
        st = sy["st"]
        return R.rows_of(st["hoods"], st["nk"], st["slots"] if slots is None else slots, st["own"] if own is None else own,
                         st["own_mask"], st["pts"])
    n = sy["n"]
    if slots is None:
        import _adjoint_ref as AD
        g = np.ascontiguousarray(np.broadcast_to(sy["rows"][0], (n, sy["rows"].shape[-1])))
        ref = AD.adjoint_ref(sy["dim"], sy["order"], np.ascontiguousarray(sy["S"][sy["hoods"]]), sy["nk"], sy["S"], sy["knowns"], sy["wm"], g)
        slots, own = ref["grad_fk"][None], ref["grad_fi"][None, :, 0]
    return R.rows_of(sy["hoods"], sy["nk"], slots, own, np.ones(n, bool), np.arange(n))


def m_rows(rows, diag, scale, o=0):
    """M_rows of M = diag(d) + scale A_o, A's rows as tests/_stencil_ref.rows_of gives them.  c * value is one rounding, as in the kernel."""
    n = len(rows)
    d = np.asarray(diag, np.float64) if np.ndim(diag) else np.full(n, float(diag))
    return [(float(d[j]), [(int(c), float(scale * v[o])) for c, v in rows[j]]) for j in range(n)]


def dense_m(M_rows):
    n = len(M_rows)
    M = np.zeros((n, n))
    for r, (d, entries) in enumerate(M_rows):
        M[r, r] += d
        for c, t in entries:
            M[r, c] += t
    return M


def slots_of(M_rows, i):
    """(columns of the slots of row i, live mask): slot 0 the diagonal, slot k entry k - 1; dead where an earlier slot names the column."""
    cols = [i] + [c for c, _ in M_rows[i][1]]
    return cols, [k == 0 or cols[k] not in cols[:k] for k in range(len(cols))]


def _local_block(M_rows, J):
    """(B, number, raw): the rows J of M dense over the columns they name (the sums of one column in entry order, the diagonal first), the
    local number of every column, and per row its entries as stored: (local columns, values), the diagonal first."""
    number = {}
    raw = []
    for r in J:
        d, entries = M_rows[r]
        for c, t in entries:                                             # an own entry belongs to the diagonal: added in entry order
            if c == r:
                d = d + t
        cs, ts = [r] + [c for c, _ in entries if c != r], [d] + [t for c, t in entries if c != r]
        for c in cs:
            number.setdefault(c, len(number))
        raw.append((np.array([number[c] for c in cs]), np.array(ts)))
    B = np.zeros((len(J), len(number)))
    for a, (cs, ts) in enumerate(raw):
        for c, t in zip(cs, ts):
            B[a, c] += t                                                  # 0.0 + t = t: the first entry is stored, the later ones added
    return B, number, raw


def ldlt_solve(G, rhs):
    """(q, usable): G q = rhs by the right-looking L D L^T of the kernel, on the lower triangle of G; usable False at a pivot that is
    not positive and finite."""
    n = len(rhs)
    G, y = np.array(G, np.float64), np.array(rhs, np.float64)
    with np.errstate(all="ignore"):
        for k in range(n):
            dk = G[k, k]
            if not (dk > 0.0 and np.isfinite(dk)):
                return np.zeros(n), False
            l = G[k + 1:, k] / dk
            G[k + 1:, k + 1:] -= np.tril(np.outer(l, G[k + 1:, k]))
            y[k + 1:] -= l * y[k]
            G[k + 1:, k] = l
        q = y / np.diag(G)
        for k in range(n - 1, 0, -1):
            q[:k] -= G[k, :k] * q[k]
    return q, bool(np.isfinite(q).all())


def row_ref(M_rows, i, gram=True):
    """dict(cols, live, lstsq, gram, usable, cond): row i of Q by both statements, per slot (0.0 in the dead ones), and cond_2 of its
    Gram matrix.  gram=False: the lstsq statement alone (what a solve's reference takes)."""
    cols, live = slots_of(M_rows, i)
    J = [c for c, ok in zip(cols, live) if ok]
    B, number, raw = _local_block(M_rows, J)
    e = np.zeros(B.shape[1])
    e[number[i]] = 1.0
    q_ls = np.linalg.lstsq(B.T, e, rcond=None)[0]
    if not gram:
        out_ls = np.zeros(len(cols))
        out_ls[np.array(live)] = q_ls
        return dict(cols=cols, live=live, lstsq=out_ls)
    ns = len(J)
    G = np.zeros((ns, ns))
    for a, (cs, ts) in enumerate(raw):
        G[a, :a + 1] = np.cumsum(ts[:, None] * B[:a + 1, cs].T, axis=0)[-1]         # cumsum: strictly in entry order
    rhs = B[:, number[i]].copy()
    q_g, usable = ldlt_solve(G, rhs)
    Gs = np.tril(G) + np.tril(G, -1).T
    with np.errstate(all="ignore"):
        cond = np.linalg.cond(Gs) if np.isfinite(Gs).all() else np.inf
    out_ls, out_g = np.zeros(len(cols)), np.zeros(len(cols))
    out_ls[np.array(live)], out_g[np.array(live)] = q_ls, q_g
    return dict(cols=cols, live=live, lstsq=out_ls, gram=out_g, usable=usable, cond=cond)


def approximate_inverse_ref(M_rows, rows=None, gram=True):
    """[row_ref(M_rows, i, gram) for the rows asked for (default: all)]."""
    return [row_ref(M_rows, i, gram) for i in (range(len(M_rows)) if rows is None else rows)]


def dense_q(ref, n, which="lstsq"):
    """Q dense from approximate_inverse_ref's rows (all of them)."""
    Q = np.zeros((n, n))
    for i, row in enumerate(ref):
        for c, q in zip(row["cols"], row[which]):
            Q[i, c] += q
    return Q


def gap(row, q):
    """|q - the Gram statement's| in the unit eps cond_2(G_i) max |q_i| in which a row of Q is held."""
    scale = EPS * row["cond"] * np.abs(row["gram"]).max()
    err = np.abs(np.asarray(q) - row["gram"]).max()
    return 0.0 if err == 0.0 else err / scale


def solve_ref(M, b, Q, method, cap=20000, reverse=False):
    """(x, iterations, status, history) of the reference recurrence of `method` from zero at rtol 1e-10 with P = Q (dense); reverse: on
    the system with rows and columns reversed, another order of every sum."""
    import _krylov_block_ref as KB
    n = len(b)
    if reverse:
        M, b, Q = M[::-1, ::-1], b[::-1], Q[::-1, ::-1]
    run = L2.bicgstab2_ref if method == "bicgstab2" else KB.bicgstab_block_ref
    x, its, status, hist = run(M, b, np.zeros(n), lambda z: Q @ z, KR.RTOL, 0.0, cap)
    return (x[::-1] if reverse else x), its, status, hist


# The worst gap of the lstsq statement to the Gram statement over the rows of the systems that the GPU tests take (Q_SYSTEMS, CAPS and
# HEADLINE), as tests/test_krylov_spai_host.py measures it (17.2 when the constant was set, on 2D-tau0.25-n1000, whose Gram matrices have
# cond_2 31 at the most: there the unit is small and lstsq's own rounding shows) and holds this constant to: C0 / 4 <= measured <= C0 (the
# lstsq side depends on the LAPACK at hand).  The GPU bar is 8 times it: the margin for the device's fused multiply-adds.
C0 = 20.0

# What the GPU test compares Q on, row by row.
Q_SYSTEMS = ("2D-tau1-n130", "2D-dirichlet-n130", "3D-tau1-n130", "random-n130")

# name: {method: maxiter}: twice the reference's count.
CAPS = {
    "2D-tau0.25-n1000": {"bicgstab2": 8, "bicgstab": 6},
    "2D-tau1-n130": {"bicgstab2": 12, "bicgstab": 10},
    "2D-tau1-n1000": {"bicgstab2": 16, "bicgstab": 16},
    "2D-dirichlet-n1000": {"bicgstab2": 52, "bicgstab": 54},
    "random-n130": {"bicgstab2": 8, "bicgstab": 8},
}

# The systems that no other preconditioner of the solver reaches: name: {method: maxiter}.  (Blocks of 16: 886 iterations of BiCGSTAB(2)
# on the first, and status 2 from BiCGSTAB on the second.)
HEADLINE = {
    "3D-tau1-n1000": {"bicgstab2": 76, "bicgstab": 76},
    "3D-tau1-n2000": {"bicgstab2": 132, "bicgstab": 144},
}

# The transposed solve of the GPU tests: (name, maxiter), twice bicgstab2_ref's count on M^T with Q^T.
TRANSPOSED = ("2D-dirichlet-n130", 16)

# (name, method) pairs whose count under the reversed summation order leaves 1.25x of the plain one: off the GPU list.
HOST_ONLY = []
GPU_CASES = [(name, method) for name, caps in CAPS.items() for method in caps if (name, method) not in HOST_ONLY]
