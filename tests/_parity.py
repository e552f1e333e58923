"""Parity helpers shared by the CPU and GPU tests.

`truth_fit` is an independent extended-precision (x87 long double, eps = 5.4e-20) statement of
the WLSQM fit in numpy: it gives the noise floor of ANY fp64 implementation on a given input, so a
parity tolerance can be tied to what double precision can resolve at all.

Parity metric: per DOF column m over the batch,
    E_m = max_j |fi[j,m] - ref[j,m]| / max_j |ref[j,m]|.
The north-star tolerance is E_m <= 1e-10.  Where the fit itself is ill-conditioned in fp64 (tiny
neighbourhoods, high derivatives: the REFERENCE's own error against the extended-precision
solution, N_m, exceeds 1e-10) no two fp64 implementations can agree to 1e-10 unless they replay
each other's roundoff, so the asserted bound is  E_m <= 1e-10 + NOISE_MULT * N_m  and the test
additionally requires the candidate to be no further from the truth than the reference is (same
multiplier).  Known DOFs must be bit-identical to the input.
"""
from typing import NamedTuple

import numpy as np

TOL = 1e-10
NOISE_MULT = 8.0
# Additive floor of the per-case criterion (assert_per_case), for families on which the reference happens to be exact (q = 0).  Derived
# from the CPU rehearsal (tests/test_adversarial_cpu.py) as the smallest value that lets the emulated fast arithmetic pass: no family
# needs one.  The candidate for it, exactpoly_grid (a dyadic polynomial on a lattice), still leaves the oracle at q >= 2.7e2 because the
# weights' square roots are inexact; the smallest oracle q of any family is 1e-2 (collinear, 3D order 4), where the emulation is at 0.3x.
Q_FLOOR = 0.0

_P2 = [(0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2), (3, 0), (2, 1), (1, 2), (0, 3),
       (4, 0), (3, 1), (2, 2), (1, 3), (0, 4)]
_P3 = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1),
       (2, 0, 0), (1, 1, 0), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 1),
       (3, 0, 0), (2, 1, 0), (1, 2, 0), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3), (1, 0, 2), (2, 0, 1), (1, 1, 1),
       (4, 0, 0), (3, 1, 0), (2, 2, 0), (1, 3, 0), (0, 4, 0), (0, 3, 1), (0, 2, 2), (0, 1, 3), (0, 0, 4),
       (1, 0, 3), (2, 0, 2), (3, 0, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2)]
_FACT = [1.0, 1.0, 2.0, 6.0, 24.0]
_NDOF = {1: [1, 2, 3, 4, 5], 2: [1, 3, 6, 10, 15], 3: [1, 4, 10, 20, 35]}


def exponents(dim, order):
    no = _NDOF[dim][order]
    if dim == 1:
        return [(a,) for a in range(no)]
    return (_P2 if dim == 2 else _P3)[:no]


def truth_fit(dim, xk, fk, nk, xi, fi_in, order, knowns, wm):
    """Extended-precision WLSQM fit of a batch (same argument meaning as fit_*D_many).  1D: xk (n,K),
    xi (n,).  Returns fi (n, max_no) float64 (knowns copied from fi_in).  Independent of oracle/."""
    LD = np.longdouble
    n = len(nk)
    out = np.array(fi_in, dtype=np.float64, copy=True)
    for j in range(n):
        o, nkj, kn = int(order[j]), int(nk[j]), int(knowns[j])
        ex = exponents(dim, o)
        no = len(ex)
        unknown = [a for a in range(no) if not (kn >> a) & 1]
        extra = bin(kn >> no).count("1")                      # infra.pyx:119-121 quirk: stray high bits drop unknowns
        if extra:
            unknown = unknown[:max(len(unknown) - extra, 0)]
        if not unknown:
            continue
        if dim == 1:
            d = (np.asarray(xk[j, :nkj], LD) - LD(xi[j]))[:, None]
        else:
            d = np.asarray(xk[j, :nkj, :dim], LD) - np.asarray(xi[j, :dim], LD)[None, :]
        Cm = np.ones((nkj, no), LD)
        for a, e in enumerate(ex):
            for m, p in enumerate(e):
                if p:
                    Cm[:, a] *= d[:, m] ** p / LD(_FACT[p])
        if int(wm[j]) == 1:
            w = np.ones(nkj, LD)
        else:
            d2 = (d * d).sum(axis=1)
            t = LD(1) - np.sqrt(d2 / d2.max())
            w = LD(1e-4) + (LD(1) - LD(1e-4)) * t * t
        f = np.asarray(fk[j, :nkj], LD).copy()
        dropped = [a for a in range(no) if not (kn >> a) & 1 and a not in unknown]
        for a in range(no):
            if (kn >> a) & 1:
                f -= Cm[:, a] * LD(fi_in[j, a])               # known DOFs move to the right-hand side
        Cu = Cm[:, unknown]
        # column equilibration (exact in effect; keeps the elimination well scaled), then normal equations
        s = np.sqrt((w[:, None] * Cu * Cu).sum(axis=0))
        s[s == 0] = 1
        Cs = Cu / s
        A = (Cs * w[:, None]).T @ Cs
        b = (Cs * w[:, None]).T @ f
        x = _solve_ld(A, b) / s
        out[j, unknown] = x.astype(np.float64)
        del dropped
    return out


def _unknown_set(dim, o, kn):
    """(no, unknown, known, dropped) of one case: the DOFs the fit solves for, the true knowns and the unknowns that stray high mask bits
    drop (infra.pyx:119-121)."""
    no = len(exponents(dim, o))
    unknown = [a for a in range(no) if not (kn >> a) & 1]
    extra = bin(kn >> no).count("1")                          # infra.pyx:119-121 quirk: stray high bits drop unknowns
    kept = unknown[:max(len(unknown) - extra, 0)] if extra else unknown
    return no, kept, [a for a in range(no) if (kn >> a) & 1], unknown[len(kept):]


def _system_mp(dim, xk, nk, xi, order, knowns, wm, j):
    """Case j of a batch in mpmath (inside mp.workdps): None when it has nothing to solve, else a dict with
      no, unknown, known, dropped   the DOF classes,
      C[k][a]                       the design matrix (scaled monomials of the offsets), all `no` columns,
      w[k]                          the weights,
      s[i]                          the column equilibration of the unknowns (sqrt of sum_k w c^2; 1 for a zero column),
      cols[i][k], wc[i][k]          the equilibrated columns of the unknowns and the same times w,
      A                             the equilibrated normal matrix  cols^T W cols,
      kappa                         the 2-norm condition number of sqrt(W) cols (fp64 numpy).
    The one statement of the fit's matrix that truth_fit_mp and truth_operator_mp share."""
    from mpmath import mp, mpf
    one, w0 = mpf(1), mpf(1e-4)
    fact = [mpf(v) for v in _FACT]
    o, nkj, kn = int(order[j]), int(nk[j]), int(knowns[j])
    ex = exponents(dim, o)
    no, unknown, known, dropped = _unknown_set(dim, o, kn)
    if not unknown:
        return None
    if dim == 1:
        d = [[mpf(float(xk[j, k])) - mpf(float(xi[j]))] for k in range(nkj)]
    else:
        d = [[mpf(float(xk[j, k, m])) - mpf(float(xi[j, m])) for m in range(dim)] for k in range(nkj)]
    C = []
    for k in range(nkj):
        pw = [[one, dk, dk * dk, dk ** 3, dk ** 4] for dk in d[k]]
        row = []
        for e in ex:
            v = one
            for m, p in enumerate(e):
                if p:
                    v = v * pw[m][p] / fact[p]
            row.append(v)
        C.append(row)
    if int(wm[j]) == 1:
        w = [one] * nkj
    else:
        d2 = [mp.fsum(x * x for x in dk) for dk in d]
        dmax = max(d2)
        w = []
        for v in d2:
            t = one - mp.sqrt(v / dmax)
            w.append(w0 + (one - w0) * t * t)
    nu = len(unknown)
    cols = [[C[k][a] for k in range(nkj)] for a in unknown]
    s = [mp.sqrt(mp.fsum(w[k] * c[k] * c[k] for k in range(nkj))) for c in cols]
    s = [v if v != 0 else one for v in s]
    cols = [[c[k] / s[i] for k in range(nkj)] for i, c in enumerate(cols)]
    wc = [[w[k] * c[k] for k in range(nkj)] for c in cols]
    A = [[None] * nu for _ in range(nu)]
    for a in range(nu):
        for b in range(a, nu):
            A[a][b] = A[b][a] = mp.fdot(wc[a], cols[b])
    B = np.array([[float(mp.sqrt(w[k]) * cols[i][k]) for i in range(nu)] for k in range(nkj)])
    sv = np.linalg.svd(B, compute_uv=False)
    kappa = sv[0] / sv[-1] if sv[-1] > 0 else np.inf
    return dict(no=no, nk=nkj, unknown=unknown, known=known, dropped=dropped, C=C, w=w, s=s, cols=cols, wc=wc, A=A, kappa=kappa)


def truth_fit_mp(dim, xk, fk, nk, xi, fi_in, order, knowns, wm, dps=60, as_mp=False):
    """The WLSQM fit of a batch in mpmath at `dps` (>= 60) digits: same arguments and meaning as `truth_fit` (knowns masks, the stray-bit
    quirk, both weightings, per-case orders, the 1D layout), without its limit (x87 long double on the normal equations stops being a
    truth once the squared condition number nears 1e16; at 60 digits the normal equations lose nothing that fp64 could see).
    Returns (fi, kappa): fi (n, max_no) float64 with knowns copied from fi_in (as_mp=True: an object array of mpf instead), and per case
    kappa_j, the 2-norm condition number of the column-equilibrated design matrix of the unknowns weighted by sqrt(w) (fp64 numpy; 1.0 for
    a case with nothing to solve).  The columns are equilibrated and the right-hand side scaled before the solve, so that the elimination
    sees entries of order one whatever the length scale and the magnitude of the data are."""
    from mpmath import mp, mpf
    assert dps >= 60
    n = len(nk)
    out = np.array(fi_in, dtype=np.float64, copy=True)
    full = np.array([[mpf(float(v)) for v in row] for row in np.asarray(fi_in, np.float64)], dtype=object).reshape(out.shape) if as_mp else None
    kappa = np.ones(n)
    with mp.workdps(dps):
        one = mpf(1)
        for j in range(n):
            m = _system_mp(dim, xk, nk, xi, order, knowns, wm, j)
            if m is None:
                continue
            nkj, C = m["nk"], m["C"]
            f = [mpf(float(fk[j, k])) for k in range(nkj)]
            for a in m["known"]:                              # known DOFs move to the right-hand side
                va = mpf(float(fi_in[j, a]))
                f = [f[k] - C[k][a] * va for k in range(nkj)]
            fs = max(abs(v) for v in f)
            fs = fs if fs != 0 else one
            fsc = [v / fs for v in f]
            x = _solve_mp(m["A"], [[mp.fdot(wca, fsc)] for wca in m["wc"]])
            for i, a in enumerate(m["unknown"]):
                v = x[i][0] * fs / m["s"][i]
                out[j, a] = float(v)
                if as_mp:
                    full[j, a] = v
            kappa[j] = m["kappa"]
    return (full if as_mp else out), kappa


# classes of a DOF of one case (Operator.kind)
DOF_UNKNOWN, DOF_KNOWN, DOF_DROPPED, DOF_BEYOND = 0, 1, 2, 3


class Operator(NamedTuple):
    """What truth_operator_mp returns: (S, J, kappa) and, beside them, `live` (n, K, max_no) bool, the entries of S that the fit defines,
    and `kind` (n, max_no) int8, the class of every DOF: DOF_UNKNOWN, DOF_KNOWN, DOF_DROPPED (by stray high mask bits), DOF_BEYOND (the
    case's order).  `S, J, kappa = op[:3]` unpacks the operator alone."""
    S: np.ndarray
    J: np.ndarray
    kappa: np.ndarray
    live: np.ndarray
    kind: np.ndarray


def truth_operator_mp(dim, xk, nk, xi, order, knowns, wm, dps=60, as_mp=False):
    """The fit's linear operator in mpmath, with the conventions of truth_fit_mp (same arguments but fk / fi, which the operator does not
    see): fi_out[a] = sum_k S[k, a] fk[k] + sum_b J[a, b] fi_in[b] for every unknown a.  Returns an Operator (S, J, kappa, live, kind):
      S (n, K, max_no)       S[j, k, a] = (A_UU^-1 C_U^T W)[a, k] = d fi_a / d fk_k for a in the unknown set U and k < nk[j], 0 elsewhere
                             (`.live` marks the defined entries),
      J (n, max_no, max_no)  J[j, a, b] = -(A_UU^-1 A_U,Kn)[a, b] = d fi_a / d fi_in_b for a in U and b a true known, 0 elsewhere,
      kappa (n,)             truth_fit_mp's, from the same statement of the matrix (`_system_mp`).
    float64 arrays, or object arrays of mpf with as_mp=True (what truth_adjoint_mp takes).  One elimination per case, with nk + |Kn|
    right-hand sides: the columns of W C_U (unit data at neighbour k) and of -A_U,Kn (a unit known value moved to the right-hand side)."""
    from mpmath import mp, mpf
    assert dps >= 60
    n = len(nk)
    K = int(np.asarray(xk).shape[1])
    no_max = max(len(exponents(dim, int(o))) for o in order)
    S = np.zeros((n, K, no_max), object if as_mp else np.float64)
    J = np.zeros((n, no_max, no_max), object if as_mp else np.float64)
    live = np.zeros((n, K, no_max), bool)
    kind = np.full((n, no_max), DOF_BEYOND, np.int8)
    kappa = np.ones(n)
    with mp.workdps(dps):
        if as_mp:
            S[...] = mpf(0); J[...] = mpf(0)
        for j in range(n):
            no, unknown, known, dropped = _unknown_set(dim, int(order[j]), int(knowns[j]))
            kind[j, unknown], kind[j, known], kind[j, dropped] = DOF_UNKNOWN, DOF_KNOWN, DOF_DROPPED
            m = _system_mp(dim, xk, nk, xi, order, knowns, wm, j)
            if m is None:
                continue
            nkj, C, wc = m["nk"], m["C"], m["wc"]
            rhs = [list(wca) + [-mp.fdot(wca, [C[k][b] for k in range(nkj)]) for b in known] for wca in wc]
            x = _solve_mp(m["A"], rhs)
            for i, a in enumerate(unknown):
                xs = [v / m["s"][i] for v in x[i]]
                for k in range(nkj):
                    S[j, k, a] = xs[k] if as_mp else float(xs[k])
                for t, b in enumerate(known):
                    J[j, a, b] = xs[nkj + t] if as_mp else float(xs[nkj + t])
                live[j, :nkj, a] = True
            kappa[j] = m["kappa"]
    return Operator(S, J, kappa, live, kind)


def truth_adjoint_mp(op, g, dps=60):
    """The transpose of the fit's operator applied to g (n, >= max_no) = dL/dfi_out, contracted in mpmath from `op` =
    truth_operator_mp(..., as_mp=True) and rounded once: no fp64 cancellation in the truth.  Returns float64 (grad_fk, grad_fi, s):
      grad_fk[j, k] = sum_{a in U} S[j, k, a] g[j, a]                        (0 for k >= nk[j]),
      grad_fi[j, b] = g[j, b] + sum_{a in U} g[j, a] J[j, a, b]  for a known b,  g[j, b] for a dropped DOF,  0 for an unknown (and beyond
                      the case's order),
      s[j]          = max_k sum_{a in U} |S[j, k, a] g[j, a]|, the case's scale as tests/_adjoint_ref.contract defines it (1 where that is 0)."""
    from mpmath import mp, mpf
    S, J, kind = op.S, op.J, op.kind
    assert S.dtype == object, "truth_adjoint_mp contracts before it rounds: it takes truth_operator_mp(..., as_mp=True)"
    n, K, no_max = S.shape
    gfk, gfi, s = np.zeros((n, K)), np.zeros((n, no_max)), np.ones(n)
    with mp.workdps(dps):
        for j in range(n):
            gm = [mpf(float(g[j, a])) for a in range(no_max)]
            U = [a for a in range(no_max) if kind[j, a] == DOF_UNKNOWN]
            top = mpf(0)
            for k in range(K):
                terms = [S[j, k, a] * gm[a] for a in U]
                gfk[j, k] = float(mp.fsum(terms))
                top = max(top, mp.fsum(abs(t) for t in terms))
            if top > 0:
                s[j] = float(top)
            for b in range(no_max):
                if kind[j, b] == DOF_KNOWN:
                    gfi[j, b] = float(gm[b] + mp.fsum(gm[a] * J[j, a, b] for a in U))
                elif kind[j, b] == DOF_DROPPED:
                    gfi[j, b] = float(gm[b])
    return gfk, gfi, s


def _solve_mp(A, B):
    """Gaussian elimination with partial pivoting on lists of mpf: A (n x n; overwritten), B (n rows of m right-hand-side entries;
    overwritten).  Returns X as n rows of m."""
    n = len(B)
    m = len(B[0]) if n else 0
    for c in range(n):
        p = max(range(c, n), key=lambda r: abs(A[r][c]))
        if p != c:
            A[c], A[p] = A[p], A[c]; B[c], B[p] = B[p], B[c]
        piv = A[c][c]
        rc, bc = A[c], B[c]
        for r in range(c + 1, n):
            f = A[r][c] / piv
            if f != 0:
                rr, br = A[r], B[r]
                for t in range(c + 1, n):
                    rr[t] -= f * rc[t]
                for t in range(m):
                    br[t] -= f * bc[t]
    X = [None] * n
    for r in range(n - 1, -1, -1):
        acc = list(B[r])
        for t in range(r + 1, n):
            art, xt = A[r][t], X[t]
            for q in range(m):
                acc[q] -= art * xt[q]
        X[r] = [v / A[r][r] for v in acc]
    return X


def _solve_ld(A, b):
    """Gaussian elimination with partial pivoting in long double."""
    A = A.copy(); b = b.copy()
    n = len(b)
    for c in range(n):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        if p != c:
            A[[c, p]] = A[[p, c]]; b[[c, p]] = b[[p, c]]
        piv = A[c, c]
        for r in range(c + 1, n):
            m = A[r, c] / piv
            if m != 0:
                A[r, c:] -= m * A[c, c:]
                b[r] -= m * b[c]
    x = np.zeros(n, np.longdouble)
    for r in range(n - 1, -1, -1):
        x[r] = (b[r] - A[r, r + 1:] @ x[r + 1:]) / A[r, r]
    return x


def column_metric(a, ref):
    """E_m per column; columns whose reference is identically zero compare absolutely."""
    a = np.asarray(a, np.float64); ref = np.asarray(ref, np.float64)
    scale = np.nanmax(np.abs(ref), axis=0)
    scale = np.where(scale > 0, scale, 1.0)
    with np.errstate(invalid="ignore"):
        return np.nanmax(np.abs(a - ref), axis=0) / scale


def assert_parity(cand, ref, truth=None, what="", tol=TOL, noise_mult=NOISE_MULT):
    """Assert the column metric; with `truth`, allow the reference's own fp64 noise floor."""
    cand = np.asarray(cand); ref = np.asarray(ref)
    assert cand.shape == ref.shape, (cand.shape, ref.shape)
    if not np.array_equal(np.isnan(cand), np.isnan(ref)):
        where = np.argwhere(np.isnan(cand) != np.isnan(ref))[:6]
        raise AssertionError("%s: NaN pattern differs at %s: candidate %s, reference %s"
                             % (what, where.tolist(), [cand[tuple(w)] for w in where], [ref[tuple(w)] for w in where]))
    E = column_metric(cand, ref)
    bound = np.full_like(E, tol)
    if truth is not None:
        N = column_metric(ref, truth)
        bound = tol + noise_mult * N
        Ec = column_metric(cand, truth)
        assert np.all(Ec <= tol + noise_mult * N), (
            "%s: candidate further from the extended-precision solution than the reference allows: %s vs noise %s"
            % (what, Ec, N))
    assert np.all(E <= bound), "%s: column metric %s exceeds bound %s" % (what, E, bound)
    return E


def case_q(x, truth, kappa, scale=None):
    """Per-case error in units of what fp64 normal equations can resolve: q_j = max_m |x_jm - T_jm| / (s_m eps kappa_j^2), s_m the column
    scale of the truth over the batch (1 for a column that is identically zero).  NaN / inf in x give q = inf."""
    x = np.asarray(x, np.float64); truth = np.asarray(truth, np.float64)
    if scale is None:
        scale = np.nanmax(np.abs(truth), axis=0)
        scale = np.where(scale > 0, scale, 1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs(x - truth) / scale
    e = np.where(np.isfinite(e), e, np.inf)
    return e.max(axis=1) / (np.finfo(np.float64).eps * np.asarray(kappa, np.float64) ** 2)


def assert_per_case(cand, ref, truth, kappa, what="", noise_mult=NOISE_MULT, floor=None):
    """Criterion (b): max_j q_j(candidate) <= noise_mult * max_j q_j(reference) + floor.  A max over the batch of a per-case quantity that
    is already divided by the case's own conditioning: one bad lane cannot hide behind the batch's worst-conditioned case.
    Returns (q_cand_max, q_ref_max)."""
    floor = Q_FLOOR if floor is None else floor
    qc, qr = case_q(cand, truth, kappa), case_q(ref, truth, kappa)
    j = int(np.argmax(qc))
    assert qc.max() <= noise_mult * qr.max() + floor, (
        "%s: per-case error q = %.3g at case %d (kappa %.3g) exceeds %g * %.3g + %g (the reference's worst case)"
        % (what, qc.max(), j, np.asarray(kappa)[j], noise_mult, qr.max(), floor))
    return float(qc.max()), float(qr.max())


def sens_q(x, S, live, kappa):
    """case_q for sensitivities (n, K, no) against truth_operator_mp's S: q_j = max over the case's live entries of |x - S| / (s_a eps
    kappa_j^2), s_a the scale of DOF column a over the batch's live entries (1 for a column without any).  A live entry that is NaN / inf
    gives q = inf; a case without live entries has q = 0."""
    x = np.asarray(x, np.float64)[:, :, :S.shape[2]]
    scale = np.where(live, np.abs(S), 0.0).max(axis=(0, 1))
    scale = np.where(scale > 0, scale, 1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs(x - S) / scale
    e = np.where(live, np.where(np.isfinite(e), e, np.inf), 0.0)
    return e.max(axis=(1, 2)) / (np.finfo(np.float64).eps * np.asarray(kappa, np.float64) ** 2)


def grad_err(x, truth, s):
    """Per case ||x_j - truth_j||_inf / s_j (s: the case's scale, truth_adjoint_mp's); NaN / inf give inf."""
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs(np.asarray(x, np.float64) - truth).max(axis=1) / s
    return np.where(np.isfinite(e), e, np.inf)


def grad_q(x, truth, s, kappa):
    """case_q for a gradient of the adjoint: q_j = ||x_j - truth_j||_inf / (s_j eps kappa_j^2)."""
    return grad_err(x, truth, s) / (np.finfo(np.float64).eps * np.asarray(kappa, np.float64) ** 2)


def assert_q(qc, qr, kappa, what="", noise_mult=NOISE_MULT, floor=None):
    """Criterion (b) on per-case q already computed (sens_q, grad_q): max_j q_j(candidate) <= noise_mult * max_j q_j(reference) + floor."""
    floor = Q_FLOOR if floor is None else floor
    j = int(np.argmax(qc))
    assert qc.max() <= noise_mult * qr.max() + floor, (
        "%s: per-case error q = %.3g at case %d (kappa %.3g) exceeds %g * %.3g + %g (the reference's worst case)"
        % (what, qc.max(), j, np.asarray(kappa)[j], noise_mult, qr.max(), floor))
    return float(qc.max()), float(qr.max())


def assert_scaled(e_cand_ref, e_cand_truth, e_ref_truth, what="", tol=TOL, noise_mult=NOISE_MULT):
    """Criterion (a) for quantities with a per-case scale (the adjoint's gradients; grad_err): over the batch, the candidate's distance
    to the reference and to the truth are both within tol + noise_mult * N, N = max_j e_j(reference against truth)."""
    N = float(np.max(e_ref_truth))
    assert np.max(e_cand_truth) <= tol + noise_mult * N, "%s: %.3g from the truth at case %d, reference %.3g" % (
        what, np.max(e_cand_truth), int(np.argmax(e_cand_truth)), N)
    assert np.max(e_cand_ref) <= tol + noise_mult * N, "%s: %.3g from the reference at case %d, bound %.3g" % (
        what, np.max(e_cand_ref), int(np.argmax(e_cand_ref)), tol + noise_mult * N)


COND_EDGES = (1.0, 1e1, 1e2, 1e3, 1e4, 1e5)     # six bins: [1, 10), [10, 1e2), ..., [1e5, inf)


def accounting(cand, ref, truth=None, oracle=None, conds=None, known_cols=()):
    """Strict-tolerance accounting of one batch against the REFERENCE's output (SURVEY.md section 8d "Parity metric").

    Returns a JSON-able dict: per DOF column m the metric E_m of the candidate against the reference, the reference's own
    fp64 noise floor N_m (its distance to the 80-bit solution `truth`), the distance `ref_vs_oracle` between the reference
    and the bit-faithful CPU restatement of its algorithm on the same inputs (what two correct fp64 implementations of the
    SAME algorithm differ by when only the LAPACK summation order changes), how many of the unknown columns meet the strict
    north-star bound E_m <= 1e-10, and the per-case relative error binned by the reference's own condition numbers
    (ExpertSolver(debug=True).conds(), expert.pyx:429-464).  `known_cols` are excluded from the counts (they must be
    bit-identical and are asserted separately)."""
    cand = np.asarray(cand, np.float64); ref = np.asarray(ref, np.float64)
    cols = [m for m in range(ref.shape[1]) if m not in set(known_cols)]
    E = column_metric(cand, ref)
    out = {"cases": int(ref.shape[0]), "columns": len(cols), "E": [float(E[m]) for m in cols], "E_max": float(max(E[m] for m in cols)),
           "strict_1e-10_columns": int(sum(E[m] <= TOL for m in cols))}
    if truth is not None:
        N = column_metric(ref, truth); T = column_metric(cand, truth)
        out["ref_noise_floor_N"] = [float(N[m]) for m in cols]
        out["cand_vs_truth"] = [float(T[m]) for m in cols]
        out["N_max"] = float(max(N[m] for m in cols))
        out["within_1e-10_plus_8N"] = bool(all(E[m] <= TOL + NOISE_MULT * N[m] for m in cols))
        # a column the reference itself resolves to 1e-11 must meet the strict bound: anything else is a bug
        out["resolved_columns_missing_strict"] = [int(m) for m in cols if N[m] < 1e-11 and E[m] > TOL]
    if oracle is not None:
        R = column_metric(np.asarray(oracle, np.float64), ref)
        out["ref_vs_oracle"] = [float(R[m]) for m in cols]
        out["ref_vs_oracle_max"] = float(max(R[m] for m in cols))
    if conds is not None:
        scale = np.nanmax(np.abs(ref), axis=0); scale = np.where(scale > 0, scale, 1.0)
        e_case = np.nanmax(np.abs(cand - ref)[:, cols] / scale[cols], axis=1)
        conds = np.asarray(conds, np.float64)
        edges = list(COND_EDGES) + [np.inf]
        hist = []
        for lo, hi in zip(edges[:-1], edges[1:]):
            sel = (conds >= lo) & (conds < hi)
            hist.append({"cond_lo": lo, "cond_hi": (hi if np.isfinite(hi) else None), "cases": int(sel.sum()),
                         "err_median": (float(np.median(e_case[sel])) if sel.any() else None),
                         "err_max": (float(e_case[sel].max()) if sel.any() else None)})
        out["err_vs_cond"] = hist
    return out
