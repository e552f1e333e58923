"""Plain restatements of LAPACK's dgetf2 and dsytf2 (uplo = 'U') for one matrix, and the adversarial matrix families of
tests/test_gpu_lapack_edges.py.

getf2(A) / sytf2(A) run in one of two modes:
  fp64  (exact=False): IEEE double, every operation in the order of the kernel's sequential routines (seq_getf2 /
        seq_sytf2 of csrc/lapack_batched.hip, without fused multiply-adds), NaN comparisons included;
  exact (exact=True):  the same operations on fractions.Fraction.  The run also records whether every intermediate
        result was a double (`exact_ok`): when it was, every fp64 operation is exact, so the fp64 run, the kernel, and
        blocked or unblocked LAPACK must all give the same bits.
Both report the 1-based pivots in LAPACK's encoding, the factor, INFO, and every pivot decision taken:
  ("tie", step, rows)          several entries share the largest magnitude of the searched column (0-based rows for
                               getf2, 1-based for sytf2); the first one wins, as in idamax
  ("zero", step)               an exactly zero pivot (INFO)
  ("1x1", k) ("1x1_swap", k, kp) ("2x2_adj", k) ("2x2_swap", k, kp) ("ratio", k)
                               the Bunch-Kaufman branch taken at column k; "ratio" is the 1x1 accepted through
                               absakk >= alpha * colmax * (colmax / rowmax) (it is also counted as "1x1")
"""
import math
from fractions import Fraction

import numpy as np

DBL_MIN = float(np.finfo(np.float64).tiny)
EPS = float(np.finfo(np.float64).eps)
ALPHA = (1.0 + math.sqrt(17.0)) / 8.0
_FDBL_MIN = Fraction(DBL_MIN)
_FALPHA = Fraction(ALPHA)

# the kernel forms, a function of n alone (csrc/lapack_batched.hip: launch_form)
FORM_SIZES = {"lane": (1, 2, 5, 8), "group64": (9, 17, 32), "group256_lds": (33, 64, 65, 89),
              "group256_global": (90, 129, 257, 300, 512, 1024)}


def threads_of(n):
    return 1 if n <= 8 else 64 if n <= 32 else 256


class _Exact:
    """Fraction arithmetic that remembers whether every result was a double"""

    def __init__(self):
        self.ok = True

    def chk(self, v):
        if self.ok:
            try:
                self.ok = Fraction(float(v)) == v
            except OverflowError:
                self.ok = False
        return v


def _to_fraction(A):
    F = np.empty(A.shape, dtype=object)
    for idx, v in np.ndenumerate(A):
        F[idx] = Fraction(float(v))
    return F


def _idamax(col):
    """0-based idamax of a float or Fraction vector: the first largest |entry|; a NaN head wins, later NaNs never.
    Also the tied positions when several entries share the (nonzero) largest magnitude."""
    a = np.abs(col)
    if a.dtype != object:
        if np.isnan(a[0]):
            return 0, []
        a = np.where(np.isnan(a), -np.inf, a)
    p = int(np.argmax(a))                            # first occurrence
    best = a[p]
    tied = [i for i in range(len(a)) if a[i] == best] if best != 0 else []
    return p, (tied if len(tied) > 1 else [])


def getf2(A, exact=False, steps=None):
    """dgetf2 of the square A (not modified); `steps` stops after that many pivots.  Returns dict(ipiv, lu, info,
    events, exact_ok)."""
    n = A.shape[0]
    X = _Exact()
    M = _to_fraction(A) if exact else np.array(A, dtype=np.float64, order="F")
    ipiv = np.zeros(n, dtype=np.intc)
    info, events = 0, []
    with np.errstate(all="ignore"):
        for j in range(n if steps is None else min(n, steps)):
            p, tied = _idamax(M[j:, j])
            if tied:
                events.append(("tie", j, [j + t for t in tied]))
            p += j
            ipiv[j] = p + 1
            d = M[p, j]
            if d != 0:                                   # (NaN != 0)
                if p != j:
                    M[[j, p], :] = M[[p, j], :]
                if exact:
                    rows = [i for i in range(j + 1, n) if M[i, j] != 0]
                    if abs(d) >= _FDBL_MIN:
                        r = X.chk(1 / d)
                        for i in rows:
                            M[i, j] = X.chk(M[i, j] * r)
                    else:
                        for i in rows:
                            M[i, j] = X.chk(M[i, j] / d)
                elif abs(d) >= DBL_MIN:
                    M[j + 1:, j] *= 1.0 / d
                else:
                    M[j + 1:, j] /= d
            elif info == 0:
                info = j + 1
                events.append(("zero", j))
            if exact:                                    # a - 0 * u and a - l * 0 are a: only nonzero pairs move
                rows = [i for i in range(j + 1, n) if M[i, j] != 0]
                cols = [c for c in range(j + 1, n) if M[j, c] != 0]
                for c in cols:
                    u = M[j, c]
                    for i in rows:
                        M[i, c] = X.chk(M[i, c] - X.chk(M[i, j] * u))
            else:
                M[j + 1:, j + 1:] -= np.outer(M[j + 1:, j], M[j, j + 1:])
    return dict(ipiv=ipiv, lu=M, info=info, events=events, exact_ok=X.ok if exact else None)


def sytf2(A, exact=False, steps=None):
    """dsytf2 with uplo = 'U' of the upper triangle of the square A (not modified; the strict lower triangle of the
    returned factor is A's); `steps` stops after that many pivot decisions.  Returns dict(ipiv, lu, info, events, exact_ok)."""
    n = A.shape[0]
    X = _Exact()
    M = _to_fraction(A) if exact else np.array(A, dtype=np.float64, order="F")
    ipiv = np.zeros(n, dtype=np.intc)
    info, events = 0, []
    alpha = _FALPHA if exact else ALPHA

    def U(i, j):
        return M[i - 1, j - 1]

    def setU(i, j, v):
        M[i - 1, j - 1] = v

    def swap(i1, j1, i2, j2):
        t = M[i1 - 1, j1 - 1]
        M[i1 - 1, j1 - 1] = M[i2 - 1, j2 - 1]
        M[i2 - 1, j2 - 1] = t

    def absmax_first(vals):                              # |vals[0]|, then `v > best` in order (later NaNs skipped)
        best = abs(vals[0])
        for v in vals[1:]:
            if abs(v) > best:
                best = abs(v)
        return best

    k = n
    with np.errstate(all="ignore"):
        while k >= 1 and (steps is None or steps > 0):
            steps = None if steps is None else steps - 1
            kstep, kp = 1, k
            absakk = abs(U(k, k))
            imax, colmax = 1, 0
            if k > 1:
                p, tied = _idamax(M[:k - 1, k - 1])
                if tied:
                    events.append(("tie", k, [1 + t for t in tied]))
                imax, colmax = p + 1, abs(U(p + 1, k))
            isnan = (not exact) and math.isnan(absakk)
            if (absakk if absakk > colmax else colmax) == 0 or isnan:
                if info == 0:
                    info = k
                events.append(("zero", k))
                kp = k
            else:
                if absakk >= alpha * colmax:
                    kp = k
                    events.append(("1x1", k))
                else:
                    rowmax = absmax_first([U(imax, j) for j in range(imax + 1, k + 1)])
                    if imax > 1:
                        cm = absmax_first([U(i, imax) for i in range(1, imax)])
                        if cm > rowmax:
                            rowmax = cm
                    if absakk >= alpha * colmax * (colmax / rowmax):
                        kp = k
                        events += [("1x1", k), ("ratio", k)]
                    elif abs(U(imax, imax)) >= alpha * rowmax:
                        kp = imax
                        events.append(("1x1_swap", k, kp))
                    else:
                        kp, kstep = imax, 2
                        events.append(("2x2_adj", k) if kp == k - 1 else ("2x2_swap", k, kp))
                kk = k - kstep + 1
                if kp != kk:
                    for i in range(1, kp):
                        swap(i, kk, i, kp)
                    for j in range(kp + 1, kk):
                        swap(j, kk, kp, j)
                    swap(kk, kk, kp, kp)
                    if kstep == 2:
                        swap(k - 1, k, kp, k)
                if kstep == 1:
                    if exact:
                        r1 = X.chk(1 / U(k, k))
                        nz = [i for i in range(1, k) if U(i, k) != 0]
                        for j in nz:                     # U(i, j) += U(i, k) * (-r1 * U(j, k)), i <= j
                            t = X.chk(-r1 * U(j, k))
                            for i in nz:
                                if i <= j:
                                    setU(i, j, X.chk(U(i, j) + X.chk(U(i, k) * t)))
                        for i in nz:
                            setU(i, k, X.chk(U(i, k) * r1))
                    elif k > 1:
                        r1 = 1.0 / U(k, k)
                        x = M[:k - 1, k - 1].copy()
                        t = -r1 * x
                        B = M[:k - 1, :k - 1]
                        upd = B + np.outer(x, t)
                        mask = np.triu(np.ones((k - 1, k - 1), bool)) & (x != 0)[None, :]
                        B[mask] = upd[mask]
                        M[:k - 1, k - 1] = x * r1
                elif k > 2:
                    if exact:
                        d12 = U(k - 1, k)
                        d22 = X.chk(U(k - 1, k - 1) / d12)
                        d11 = X.chk(U(k, k) / d12)
                        t = X.chk(1 / X.chk(X.chk(d11 * d22) - 1))
                        d12 = X.chk(t / d12)
                        m = k - 2
                        wkm1 = [X.chk(d12 * X.chk(X.chk(d11 * U(j, k - 1)) - U(j, k))) for j in range(1, m + 1)]
                        wk = [X.chk(d12 * X.chk(X.chk(d22 * U(j, k)) - U(j, k - 1))) for j in range(1, m + 1)]
                        rows = [i for i in range(1, m + 1) if U(i, k) != 0 or U(i, k - 1) != 0]
                        for j in range(1, m + 1):
                            if wk[j - 1] == 0 and wkm1[j - 1] == 0:
                                continue
                            for i in rows:
                                if i <= j:
                                    v = X.chk(U(i, j) - X.chk(U(i, k) * wk[j - 1]))
                                    setU(i, j, X.chk(v - X.chk(U(i, k - 1) * wkm1[j - 1])))
                        for j in range(1, m + 1):
                            setU(j, k, wk[j - 1])
                            setU(j, k - 1, wkm1[j - 1])
                    else:
                        d12 = U(k - 1, k)
                        d22 = U(k - 1, k - 1) / d12
                        d11 = U(k, k) / d12
                        t = 1.0 / (d11 * d22 - 1.0)
                        d12 = t / d12
                        m = k - 2
                        ck, ckm1 = M[:m, k - 1].copy(), M[:m, k - 2].copy()
                        wkm1 = d12 * (d11 * ckm1 - ck)
                        wk = d12 * (d22 * ck - ckm1)
                        B = M[:m, :m]
                        upd = (B - np.outer(ck, wk)) - np.outer(ckm1, wkm1)
                        mask = np.triu(np.ones((m, m), bool))
                        B[mask] = upd[mask]
                        M[:m, k - 1] = wk
                        M[:m, k - 2] = wkm1
            if kstep == 1:
                ipiv[k - 1] = kp
            else:
                ipiv[k - 1] = ipiv[k - 2] = -kp
            k -= kstep
    return dict(ipiv=ipiv, lu=M, info=info, events=events, exact_ok=X.ok if exact else None)


def as_float(lu):
    return np.array([[float(v) for v in row] for row in lu], dtype=np.float64) if lu.dtype == object else lu


def bits(a):
    """the bits of a float64 array, -0 folded into +0 (a zero's sign is not part of what LAPACK promises)"""
    return (np.asarray(a, dtype=np.float64) + 0.0).view(np.int64)


def tie_kinds(n, step, rows, kind):
    """which reductions of the kernel form a tie goes through: "lane" (the lane form's sequential search), "thread" (two
    rows of one thread), "lanes" (two threads of one wave), "waves" (two waves).  `rows` are the tied rows: 0-based
    rows >= step for getf2 (kind "ge"), 1-based rows 1 .. step-1 for sytf2 (kind "sy").  The winner (the first) is paired
    with every other tied row."""
    nt = threads_of(n)
    if nt == 1:
        return {"lane"}
    base = step if kind == "ge" else 1
    tid = [(r - base) % nt for r in rows]
    w = tid[0]
    out = set()
    for t in tid[1:]:
        out.add("thread" if t == w else "lanes" if t // 64 == w // 64 else "waves")
    return out


def branches(events):
    return {e[0] for e in events} - {"tie"}


# ---- matrix families ----

def dyadic(rng, shape, exps=(-1, 0, 1), zero=0.0):
    """signed powers of two 2^e, e from `exps`; a fraction `zero` of the entries is 0"""
    v = rng.choice([-1.0, 1.0], size=shape) * np.exp2(rng.choice(exps, size=shape))
    if zero:
        v[rng.random(shape) < zero] = 0.0
    return v


def _tie_distances(rng, room):
    """row distances < room that put two rows in two lanes of a wave, in two waves, and in one thread of a group"""
    out = [int(rng.integers(1, min(64, room)))] if room > 1 else []
    if room > 64:
        out.append(int(rng.integers(64, min(256, room))))
    if room > 256:
        out.append(256)
    return out


def tie_lu_matrix(rng, n, zero_pivots=0):
    """A = L0 U0 with dyadic entries: unit L0 with sparse entries of magnitude <= 1/2 and, in every column j, planted
    multipliers of magnitude exactly 1 (ties of the pivot search, mostly with the opposite sign of the pivot) at
    distances that put the tied rows in one thread (256), across lanes (1..63) and across waves (64..255); U0 with
    +-2^k diagonal and sparse dyadic entries.  `zero_pivots` diagonal entries of U0 past the first are 0: zero columns
    after the first step.  Rows are then shuffled within small windows, so some pivots swap.  Exact factorizations are
    common, not certain: keep what getf2(A, exact=True) marks exact_ok."""
    L0 = np.eye(n)
    U0 = np.triu(dyadic(rng, (n, n), exps=(-2, -1, 0), zero=0.9), 1)
    U0[np.diag_indices(n)] = dyadic(rng, n, exps=(-1, 0, 1, 2))
    if zero_pivots and n > 2:
        for j in rng.choice(np.arange(max(1, n - 4), n), size=min(zero_pivots, n - max(1, n - 4)), replace=False):
            U0[j, j] = 0.0                               # (late: fewer steps after it that could turn inexact)
    for j in range(n - 1):
        below = np.arange(j + 1, n)
        sparse = below[rng.random(below.size) < min(1.0, 2.0 / below.size)]
        L0[sparse, j] = dyadic(rng, sparse.size, exps=(-2, -1))
        for dist in _tie_distances(rng, n - j):
            if rng.random() < 0.5:
                L0[j + dist, j] = -1.0 if rng.random() < 0.75 else 1.0
    A = L0 @ U0
    perm = np.arange(n)
    for s in range(0, n, 4):                             # local shuffles: rows trade places with near neighbours
        if rng.random() < 0.3:
            w = perm[s:s + 4].copy()
            rng.shuffle(w)
            perm[s:s + 4] = w
    return np.asfortranarray(A[perm])


def tie_sy_matrix(rng, n):
    """symmetric P^T B P, B block diagonal with dyadic blocks of order 1 to 3 (zero diagonals allowed), so every
    Bunch-Kaufman branch occurs; a few 3x3 blocks sit on rows (p1, p1 + d, p3) with d from _tie_distances and hold
    entries of equal magnitude and opposite sign in column p3 (colmax ties) over a small diagonal.  Exact
    factorizations are common: keep what sytf2(A, exact=True) marks exact_ok."""
    A = np.zeros((n, n))
    free = np.ones(n, bool)
    blocks = []
    for d in _tie_distances(rng, n - 1):
        for _ in range(20):
            p1 = int(rng.integers(0, n - d - 1))
            p2 = p1 + d
            p3 = int(rng.integers(p2 + 1, n))
            if free[[p1, p2, p3]].all():
                free[[p1, p2, p3]] = False
                blocks.append(([p1, p2, p3], True))
                break
    rest = np.flatnonzero(free)
    rng.shuffle(rest)
    i = 0
    while i < rest.size:
        m = int(rng.integers(1, 4))
        blocks.append((sorted(rest[i:i + m].tolist()), False))
        i += m
    for rows, tie in blocks:
        m = len(rows)
        B = np.zeros((m, m))
        c = dyadic(rng, 3, exps=(-1, 0, 1))
        if tie:                                          # a 2x2 pivot (p1, p3) whose Schur complement on p2 is exact
            v = 2.0 * abs(c[0])
            B[0, 2], B[1, 2] = v, -v
            B[1, 1] = c[1] if rng.random() < 0.9 else 0.0
            B[2, 2] = dyadic(rng, 1, exps=(-2,), zero=0.5)[0]
        elif m == 1:
            B[0, 0] = c[0] if rng.random() < 0.95 else 0.0
        elif m == 2:                                     # zero diagonal (2x2 pivot) or one nonzero diagonal entry
            B[0, 1] = c[0]
            kind = rng.integers(3)
            if kind:
                B[kind - 1, kind - 1] = c[1] * (4.0 if rng.random() < 0.5 else 0.25)
        else:                                            # a zero-diagonal pair beside a 1x1
            B[0, 2] = c[0]
            B[1, 1] = c[1]
        B = B + np.triu(B, 1).T
        A[np.ix_(rows, rows)] = B
    return np.asfortranarray(A)


def bk_family(rng, name, n):
    """symmetric matrices that drive Bunch-Kaufman down each of its branches"""
    if n == 1:
        return np.asfortranarray(rng.standard_normal((1, 1)))
    if name == "normal":
        G = rng.standard_normal((n, n))
        return np.asfortranarray(0.5 * (G + G.T))
    if name == "zero_diag":
        G = rng.standard_normal((n, n))
        A = 0.5 * (G + G.T)
        A[np.diag_indices(n)] = 0.0
        return np.asfortranarray(A)
    if name == "arrow":
        A = np.diag(rng.standard_normal(n) * 0.1)
        A[0, 1:] = A[1:, 0] = rng.standard_normal(n - 1)
        A[-1, :-1] = A[:-1, -1] = rng.standard_normal(n - 1)
        return np.asfortranarray(A)
    if name == "dominant":
        G = rng.standard_normal((n, n))
        A = 0.5 * (G + G.T)
        A[np.diag_indices(n)] = (np.abs(A).sum(axis=1) + 1.0) * rng.choice([-1.0, 1.0], n)
        return np.asfortranarray(A)
    if name == "lead2x2":                                # the last step is a 2x2 pivot at k = 2: nothing left to update
        A = np.zeros((n, n))
        c = rng.standard_normal()
        A[0, 1] = A[1, 0] = c
        if n > 2:
            G = rng.standard_normal((n - 2, n - 2))
            B = 0.5 * (G + G.T)
            B[np.diag_indices(n - 2)] = np.abs(B).sum(axis=1) + 1.0
            A[2:, 2:] = B
        return np.asfortranarray(A)
    raise ValueError(name)


BK_FAMILIES = ("normal", "zero_diag", "arrow", "dominant", "lead2x2")
BK_BRANCHES = {"1x1", "1x1_swap", "2x2_adj", "2x2_swap", "ratio"}


def backward_errors(A, x, b):
    """normwise backward error of every system A[:, :, k] x[:, k] = b[:, k] (inf norms)"""
    r = np.einsum("ijk,jk->ik", A, x) - b
    return np.abs(r).max(axis=0) / (np.abs(A).sum(axis=1).max(axis=0) * np.abs(x).max(axis=0) + np.abs(b).max(axis=0))


def sym_from_upper(U):
    return np.triu(U) + np.triu(U, 1).T


def lu_rows(A, ipiv):
    """P A: the rows of A interchanged as dgetrf's 1-based ipiv says, in order"""
    PA = np.array(A, dtype=np.float64)
    for i, p in enumerate(ipiv):
        if p - 1 != i:
            PA[[i, p - 1]] = PA[[p - 1, i]]
    return PA


def udut(F, ipiv, parts=False):
    """U D U^T (or U and D, `parts`) from the upper-triangle factor and pivots of dsytrf (U = P(n) U(n) ... P(k) U(k) ..., k decreasing)"""
    n = F.shape[0]
    Ut = np.eye(n)
    D = np.zeros((n, n))
    k = n
    while k >= 1:
        P = np.eye(n)
        Uk = np.eye(n)
        if ipiv[k - 1] > 0:
            kp = ipiv[k - 1]
            D[k - 1, k - 1] = F[k - 1, k - 1]
            Uk[:k - 1, k - 1] = F[:k - 1, k - 1]
            P[[k - 1, kp - 1]] = P[[kp - 1, k - 1]]
            step = 1
        else:
            kp = -ipiv[k - 1]
            D[k - 2:k, k - 2:k] = [[F[k - 2, k - 2], F[k - 2, k - 1]], [F[k - 2, k - 1], F[k - 1, k - 1]]]
            Uk[:k - 2, k - 2:k] = F[:k - 2, k - 2:k]
            P[[k - 2, kp - 1]] = P[[kp - 1, k - 2]]
            step = 2
        Ut = Ut @ P @ Uk
        k -= step
    return (Ut, D) if parts else Ut @ D @ Ut.T


# ---- the exact cases both test files use (the CPU test pins them against scipy, the GPU test against the kernels) ----

TIE_KINDS_REQUIRED = {"lane": {"lane"}, "group64": {"lanes"}, "group256_lds": {"lanes", "waves"},
                      "group256_global": {"lanes", "waves", "thread"}}
EXACT_NMAX = 300                 # the exact families stop here (the Fraction runs grow with n); n >= 512 get first-step ties


def exact_tie_cases(kind, n, scale_exp=0):
    """[(A, exact restatement)] of tie_lu_matrix (kind "ge") or tie_sy_matrix ("sy") at order n, times 2^scale_exp,
    kept only when every operation is exact; deterministic in (kind, n, scale_exp)"""
    rng = np.random.default_rng([7 if kind == "ge" else 8, n, scale_exp + 2000])
    want = 1 if n >= 257 else 4
    out = []
    for t in range(10 * want):
        if len(out) == want:
            break
        if kind == "ge":
            A = tie_lu_matrix(rng, n, zero_pivots=int(t % 3 == 1))
        else:
            A = tie_sy_matrix(rng, n)
        A = np.asfortranarray(np.ldexp(A, scale_exp))
        ref = (getf2 if kind == "ge" else sytf2)(A, exact=True)
        if ref["exact_ok"]:
            out.append((A, ref))
    return out


def tie_events(kind, n, ref):
    """(tie kinds met, a zero pivot met after the first step) of one restatement run"""
    kinds = set()
    for e in ref["events"]:
        if e[0] == "tie":
            kinds |= tie_kinds(n, e[1], e[2], kind)
    later_zero = any(e[0] == "zero" and (e[1] > 0 if kind == "ge" else e[1] < n) for e in ref["events"])
    return kinds, later_zero


def first_step_tie_matrix(rng, kind, n, dist):
    """random signed matrix whose first searched column (column 1 for getf2, column n for sytf2) holds two entries
    +-2, `dist` rows apart, over entries of magnitude < 1 (and a small diagonal for sytf2).  Returns (A, the winning
    row, 0-based)."""
    A = rng.uniform(-1.0, 1.0, (n, n))
    if kind == "ge":
        r = int(rng.integers(0, n - dist))
        A[r, 0], A[r + dist, 0] = 2.0, -2.0
    else:
        A = 0.5 * (A + A.T)
        r = int(rng.integers(0, n - 1 - dist))
        A[r, n - 1] = A[n - 1, r] = 2.0
        A[r + dist, n - 1] = A[n - 1, r + dist] = -2.0
        A[n - 1, n - 1] = 0.01
    return np.asfortranarray(A), r
