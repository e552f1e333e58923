"""What ExpertSolver(debug=True).conds() computes (csrc/conds.hip), stated three times, and the input families the tests run it on.

  truth_mp    per case in mpmath at DPS digits from the fp64 inputs: the unknown set of _parity._unknown_set (stray-bit quirk included), the
              reduced normal matrix sum_k w_k c_k c_k^T with the weights of _parity._system_mp, Ruiz equilibration (row and column maxima,
              square roots) run until both corrections are below 1e-30, the singular values of the scaled matrix, kappa = s_max / s_min.
              None where nothing is left to solve (nr < 1).
  statement   the kernel's three steps in numpy fp64 with the kernel's thresholds (Ruiz: 1e-15, at most 100 sweeps; one-sided Jacobi:
              |gamma| > 1e-15 sqrt(alpha beta), at most 60 sweeps).  The CPU stand-in that tests/test_conds_host.py measures.
  reference   np.linalg.cond (LAPACK, as the reference's dgesvd) of the statement's scaled matrix.

The error of a condition number x against the truth T is counted in units of eps T^2: the smallest singular value of the scaled matrix
moves by eps s_max under fp64 rounding of the matrix, which is eps T relative to itself, so eps T^2 in the quotient.  Q_REF is the largest
such figure of `reference` over the families (recorded below; the host test holds it from both sides) and the GPU bound is
_parity.NOISE_MULT * max(1, Q_REF) units.

Families (seeded; tests/golden/conds_truth.npz holds their truths and a digest of their inputs, written by
`python tests/_conds_ref.py --write`).  The kernel runs one lane per case in 64-lane blocks:
  uniform_<dim>_<order>   all 15 pairs, 130 cases (two full blocks and two lanes; 66 where no >= 20).  xi uniform in the unit box,
                          K = 2 no + 4 neighbours within 0.1 of it, nk ragged in [nr + 2, K] with nk[0] = K, the two weightings
                          interleaved, the masks cycling through: 0; bit 0; several bits; stray bits above no; all but one DOF (nr == 1);
                          the full mask (nr < 1).
  mixed_<dim>             the sweep goldens as they are: order, mask, weighting and nk per case.
  chunks                  1D, K = 8, orders 0..4 per case, 130 cases; the GPU test repeats them with period 130 to 32768 + 130 cases.
  degenerate              2D order 2, 130 cases; every fourth is degenerate: all neighbours on a line through xi, every neighbour a copy
                          of one point, or nk = nr - 1.
  balanced                1D order 1, 130 cases of neighbours in pairs about xi but for 2^-25 .. 2^-36: nearly orthogonal columns, the edge
                          of the Jacobi rotation test (on the other families a threshold of 1e-9 changes nothing fp64 can see: the
                          error of a skipped rotation is of second order unless two singular values coincide).
A neighbourhood of a generated family whose fp64 condition number (`reference`) exceeds KAPPA_DRAW is drawn again from the same stream:
at nk = nr + 2 a random cloud is now and then within rounding of singular, and the families are to hold regular cases only
(the truth of every one is asserted <= KAPPA_MAX by the host test)."""
import hashlib
import io
import os
import sys
import zipfile

import numpy as np

import _cases as K
import _parity as P

EPS = float(np.finfo(np.float64).eps)
DPS = 50
RUIZ_TRUTH = 1e-30
RUIZ_TRUTH_SWEEPS = 1000
KAPPA_MAX = 1e8                    # every regular case of a generated family (the host test asserts it on the truth)
KAPPA_DRAW = 2e7                   # the generators' own redraw threshold, on the fp64 figure: a factor 5 below KAPPA_MAX
NO_DIGITS = 1.0 / 64               # a truth with kappa eps >= this (or infinite) says nothing about an fp64 value: the degenerate class
HUGE = 2.0 ** 40                   # what the kernel must at least report there
# Largest |reference - truth| / (eps truth^2) over all families, as tests/test_conds_host.py measures it (it prints the figure per family
# and holds this constant to Q_REF / 4 <= measured <= Q_REF).  Measured: 2.00 (balanced: two ulps of a value
# next to 1; 1.84 on chunks); the statement's own figure is the same.
Q_REF = 2.3
FIXTURE = os.path.join(K.GOLDEN, "conds_truth.npz")
DIMS_ORDERS = [(d, o) for d in (1, 2, 3) for o in range(5)]


# ---------------------------------------------------------------------------------------------------------------- the three statements
def truth_case(dim, xk, nk, xi, order, knowns, wm, j):
    """kappa of case j as an mpf (mp.inf for a singular matrix), None for nr < 1.  Call inside mp.workdps(DPS)."""
    from mpmath import mp, mpf
    m = P._system_mp(dim, xk, nk, xi, order, knowns, wm, j)
    if m is None:
        return None
    C, w, U, nkj = m["C"], m["w"], m["unknown"], m["nk"]
    nr = len(U)
    A = [[None] * nr for _ in range(nr)]
    for a in range(nr):
        wa = [w[k] * C[k][U[a]] for k in range(nkj)]
        for b in range(a, nr):
            A[a][b] = A[b][a] = mp.fsum(wa[k] * C[k][U[b]] for k in range(nkj))
    r, c = [mpf(1)] * nr, [mpf(1)] * nr
    tol = mpf(RUIZ_TRUTH)
    for _ in range(RUIZ_TRUTH_SWEEPS):
        dr = [mp.sqrt(max(abs(A[i][t] / (r[i] * c[t])) for t in range(nr))) for i in range(nr)]
        dc = [mp.sqrt(max(abs(A[i][t] / (r[i] * c[t])) for i in range(nr))) for t in range(nr)]
        if min(dr) == 0 or min(dc) == 0:
            return mp.inf                                       # a zero row: nothing to equilibrate, no smallest singular value
        r = [r[i] * dr[i] for i in range(nr)]
        c = [c[t] * dc[t] for t in range(nr)]
        if max(abs(1 - v * v) for v in dr) < tol and max(abs(1 - v * v) for v in dc) < tol:
            break
    S = mp.matrix([[A[i][t] / (r[i] * c[t]) for t in range(nr)] for i in range(nr)])
    sv = mp.svd_r(S, compute_uv=False)
    smax, smin = max(sv), min(sv)
    return mp.inf if smin <= 0 else smax / smin


def truth_mp(dim, xk, nk, xi, order, knowns, wm, cases=None):
    """[kappa_j as mpf, or None for nr < 1] over `cases` (default: all)."""
    from mpmath import mp
    with mp.workdps(DPS):
        return [truth_case(dim, xk, nk, xi, order, knowns, wm, j) for j in (range(len(nk)) if cases is None else cases)]


def split(kappa):
    """(hi, lo) doubles of an mpf with hi + lo = kappa to about 1e-32 relative; (nan, 0) for None, (inf, 0) beyond fp64."""
    from mpmath import mp, mpf
    if kappa is None:
        return np.nan, 0.0
    with mp.workdps(DPS):
        if not mp.isfinite(kappa) or kappa > mpf(1e300):
            return np.inf, 0.0
        hi = float(kappa)
        return hi, float(kappa - mpf(hi))


def _scaled_matrix(dim, xk, nk, xi, order, knowns, wm, j):
    """Steps 1 and 2 of the kernel in fp64: the Ruiz-scaled reduced normal matrix of case j (None for nr < 1)."""
    o, nkj = int(order[j]), int(nk[j])
    ex = P.exponents(dim, o)
    _, U, _, _ = P._unknown_set(dim, o, int(knowns[j]))
    nr = len(U)
    if nr < 1:
        return None
    d = (xk[j, :nkj] - xi[j]).reshape(nkj, dim)
    c = np.ones((nkj, len(ex)))
    for a, e in enumerate(ex):
        for m, p in enumerate(e):
            if p:
                c[:, a] *= d[:, m] ** p / P._FACT[p]
    d2 = (d * d).sum(axis=1)
    if int(wm[j]) == 1:
        w = np.ones(nkj)
    else:
        t = 1.0 - np.sqrt(d2 / d2.max()) if nkj else d2
        w = 1e-4 + (1.0 - 1e-4) * t * t
    cu = c[:, U]
    A = np.zeros((nr, nr))
    for k in range(nkj):                                        # the kernel's order of summation: neighbour by neighbour
        A += w[k] * np.outer(cu[k], cu[k])
    rp, cp, rs, cs = np.ones(nr), np.ones(nr), np.ones(nr), np.ones(nr)
    for _ in range(100):
        M = np.abs(A / (rp[:, None] * cp[None, :]))
        dr, dc = np.sqrt(M.max(axis=1)), np.sqrt(M.max(axis=0))
        rp *= dr; rs /= dr; cp *= dc; cs /= dc
        if np.abs(1.0 - dr * dr).max() < 1e-15 and np.abs(1.0 - dc * dc).max() < 1e-15:
            break
    return A * rs[:, None] * cs[None, :]


def _jacobi_cond(G, tol=1e-15):
    """Step 3: one-sided Jacobi on the columns of G (overwritten), s_max / s_min of the column norms.  `tol` is the kernel's rotation
    threshold; the host test passes another one to show that the `balanced` family tells the two apart."""
    nr = G.shape[0]
    for _ in range(60):
        rotated = False
        for p in range(nr - 1):
            for q in range(p + 1, nr):
                ap, aq = G[:, p].copy(), G[:, q].copy()
                alpha, beta, gamma = ap @ ap, aq @ aq, ap @ aq
                if abs(gamma) > tol * np.sqrt(alpha * beta) and gamma != 0.0:
                    zeta = (beta - alpha) / (2.0 * gamma)
                    t = (1.0 if zeta >= 0.0 else -1.0) / (abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                    cs = 1.0 / np.sqrt(1.0 + t * t)
                    sn = cs * t
                    G[:, p] = cs * ap - sn * aq
                    G[:, q] = sn * ap + cs * aq
                    rotated = True
        if not rotated:
            break
    s = np.sqrt((G * G).sum(axis=0))
    return s.max() / s.min()


def statement(dim, xk, nk, xi, order, knowns, wm, jacobi_tol=1e-15):
    """The kernel's three steps in numpy fp64, per case; NaN for nr < 1."""
    out = np.full(len(nk), np.nan)
    with np.errstate(all="ignore"):
        for j in range(len(nk)):
            S = _scaled_matrix(dim, xk, nk, xi, order, knowns, wm, j)
            if S is not None:
                out[j] = _jacobi_cond(S, jacobi_tol)
    return out


def reference(dim, xk, nk, xi, order, knowns, wm):
    """np.linalg.cond of the statement's scaled matrix, per case; NaN for nr < 1, inf where LAPACK cannot tell."""
    out = np.full(len(nk), np.nan)
    with np.errstate(all="ignore"):
        for j in range(len(nk)):
            S = _scaled_matrix(dim, xk, nk, xi, order, knowns, wm, j)
            if S is not None:
                out[j] = np.linalg.cond(S) if np.isfinite(S).all() else np.inf
    return out


def sweep_reference(dim):
    """The reference's own figure of the sweep golden: _cases.scaled_cond per case, NaN for nr < 1."""
    g = K.sweep(dim)
    out = np.full(len(g["nk"]), np.nan)
    for j in range(len(out)):
        o, kn = int(g["order"][j]), int(g["knowns"][j])
        if P._unknown_set(dim, o, kn)[1]:
            out[j] = K.scaled_cond(g, j, K.NDOF[dim][o], kn)
    return out


def q_units(x, truth):
    """|x - truth| / (eps truth^2) per case; inf for a non-finite x."""
    with np.errstate(all="ignore"):
        q = np.abs(np.asarray(x, np.float64) - truth) / (EPS * truth * truth)
    return np.where(np.isfinite(q), q, np.inf)


# ---------------------------------------------------------------------------------------------------------------------- the families
MASK_KINDS = ("none", "bit0", "several", "stray", "one_left", "full")


def mask(kind, no, j):
    """The knowns mask of kind `kind` (an index into MASK_KINDS) for `no` DOFs; j varies the DOF that 'one_left' keeps."""
    full = (1 << no) - 1
    if kind == 0:
        return 0
    if kind == 1:
        return 1
    if kind == 2:                                               # several bits, as many as `no` has room for beside an unknown
        bits = {1, no // 2, no - 1} if no >= 4 else ({1, 2} if no == 3 else ({1} if no == 2 else set()))
        return sum(1 << b for b in bits)
    if kind == 3:                                               # stray bits above no: each drops the last unknown left
        return (2 | 1 << (no + 1) | 1 << (no + 9)) if no >= 4 else 1 << (no + 1)
    if kind == 4:
        return full ^ (1 << ((j // 6) % no))
    return full


def _nr(dim, order, kn):
    return len(P._unknown_set(dim, int(order), int(kn))[1])


def _batch(dim, rng, n, Kn, order, knowns, wm, lo_extra=2):
    """xi uniform in the unit box, Kn neighbours within 0.1 of it, nk ragged in [nr + lo_extra, Kn] with nk[0] = Kn; a neighbourhood
    whose fp64 condition number exceeds KAPPA_DRAW is drawn again."""
    xi = rng.uniform(0.0, 1.0, (n, dim))
    xk = xi[:, None, :] + 0.1 * rng.uniform(-1.0, 1.0, (n, Kn, dim))
    nr = np.array([_nr(dim, order[j], knowns[j]) for j in range(n)])
    nk = np.array([rng.integers(min(nr[j] + lo_extra, Kn), Kn + 1) for j in range(n)], np.int32)
    nk[0] = Kn
    f = dict(dim=dim, xi=xi, xk=xk, nk=nk, order=order, knowns=knowns, wm=wm)
    for j in range(n):
        for _ in range(100):
            S = _scaled_matrix(dim, xk, nk, xi, order, knowns, wm, j)
            if S is None or np.linalg.cond(S) <= KAPPA_DRAW:
                break
            xk[j] = xi[j] + 0.1 * rng.uniform(-1.0, 1.0, (Kn, dim))
        else:
            raise AssertionError("no regular neighbourhood for case %d" % j)
    return f


def _flat(f):
    """The arrays as the API takes them: the 1D layout drops the coordinate axis."""
    if f["dim"] == 1:
        f["xi"], f["xk"] = np.ascontiguousarray(f["xi"][:, 0]), np.ascontiguousarray(f["xk"][..., 0])
    f["degenerate"] = f.get("degenerate", np.zeros(len(f["nk"]), bool))
    return f


def _uniform(dim, order):
    no = K.NDOF[dim][order]
    n = 66 if no >= 20 else 130
    rng = np.random.default_rng(1000 + 10 * dim + order)
    j = np.arange(n)
    knowns = np.array([mask(t % 6, no, t) for t in j], np.int64)
    wm = (1 + (j + j // 6) % 2).astype(np.int32)                 # both weightings under every kind of mask
    return _flat(_batch(dim, rng, n, 2 * no + 4, np.full(n, order, np.int32), knowns, wm))


def _mixed(dim):
    g = K.sweep(dim)
    return dict(dim=dim, xi=g["xi"], xk=g["xk"], nk=g["nk"], order=g["order"], knowns=g["knowns"], wm=g["wm"],
                degenerate=np.zeros(len(g["nk"]), bool))


def _chunks():
    n = 130
    rng = np.random.default_rng(2001)
    order = rng.integers(0, 5, n).astype(np.int32)
    j = np.arange(n)
    knowns = np.array([mask(t % 6, K.NDOF[1][int(order[t])], t) for t in j], np.int64)
    wm = (1 + (j + j // 6) % 2).astype(np.int32)
    return _flat(_batch(1, rng, n, 8, order, knowns, wm))


def _balanced():
    """1D order 1, 8 neighbours in four pairs xi +- h with one of them moved by 2^-e, e in 25 .. 36, all on a dyadic grid so that the
    offsets and their sum are exact in fp64: the two columns of the scaled matrix are orthogonal but for a correlation rho of 1e-13 .. 1e-7
    and kappa = (1 + rho) / (1 - rho).  A rotation threshold above rho returns 1.0, wrong by 2 rho: up to 1e9 units of eps kappa^2."""
    n = 130
    rng = np.random.default_rng(2003)
    xi = rng.integers(1, 1024, (n, 1)) / 1024.0
    h = rng.integers(8, 103, (n, 4)) / 1024.0                     # 0.008 .. 0.1
    xk = np.concatenate([xi + h, xi - h], axis=1)
    xk[:, 0] += 2.0 ** -(25 + np.arange(n) % 12)
    j = np.arange(n)
    return _flat(dict(dim=1, xi=xi, xk=xk[:, :, None], nk=np.full(n, 8, np.int32), order=np.ones(n, np.int32),
                      knowns=np.zeros(n, np.int64), wm=(1 + (j // 12) % 2).astype(np.int32)))


def _degenerate():
    n, Kn = 130, 16
    rng = np.random.default_rng(2002)
    j = np.arange(n)
    knowns = np.where(j % 8 == 3, 1, 0).astype(np.int64)
    wm = (1 + (j // 2) % 2).astype(np.int32)
    f = _batch(2, rng, n, Kn, np.full(n, 2, np.int32), knowns, wm)
    deg = j % 4 == 1
    for t in np.flatnonzero(deg):
        kind = (t // 4) % 3
        if kind == 0:                                           # on a line through xi
            a = rng.uniform(0.0, 2.0 * np.pi)
            f["xk"][t] = f["xi"][t] + rng.uniform(-0.1, 0.1, (Kn, 1)) * np.array([np.cos(a), np.sin(a)])
        elif kind == 1:                                         # copies of one point
            f["xk"][t] = f["xi"][t] + rng.uniform(0.02, 0.1, 2)
        else:                                                   # one neighbour short of the unknowns
            f["nk"][t] = _nr(2, 2, knowns[t]) - 1
    f["degenerate"] = deg
    return _flat(f)


_FAMILIES = {}


def names():
    return (["uniform_%d_%d" % do for do in DIMS_ORDERS] + ["mixed_%d" % d for d in (1, 2, 3)] + ["chunks", "degenerate", "balanced"])


def family(name):
    """dict(dim, xi, xk, nk, order, knowns, wm, degenerate) of one family; built once, never modified."""
    if name not in _FAMILIES:
        part = name.split("_")
        f = (_uniform(int(part[1]), int(part[2])) if part[0] == "uniform" else _mixed(int(part[1])) if part[0] == "mixed"
             else _chunks() if name == "chunks" else _balanced() if name == "balanced" else _degenerate())
        for v in f.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _FAMILIES[name] = f
    return _FAMILIES[name]


def args(f, sel=slice(None)):
    """The positional arguments of truth_mp / statement / reference."""
    return f["dim"], f["xk"][sel], f["nk"][sel], f["xi"][sel], f["order"][sel], f["knowns"][sel], f["wm"][sel]


def digest():
    h = hashlib.sha256()
    for name in names():
        f = family(name)
        for key in ("xi", "xk", "nk", "order", "knowns", "wm"):
            h.update(np.ascontiguousarray(f[key]).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def offsets():
    sizes = [len(family(name)["nk"]) for name in names()]
    return dict(zip(names(), np.concatenate([[0], np.cumsum(sizes)[:-1]]))), int(sum(sizes))


_TRUTH = {}


def truth(name):
    """(hi, lo) of the family's truths from the fixture: NaN for nr < 1, inf for a singular matrix; the digest is checked once."""
    if not _TRUTH:
        g = np.load(FIXTURE)
        assert np.array_equal(g["digest"], digest()), \
            "the families differ from the inputs conds_truth.npz was computed on (numpy difference on this host?)"
        off, total = offsets()
        assert g["hi"].shape == (total,) and g["lo"].shape == (total,)
        for nm in names():
            n = len(family(nm)["nk"])
            _TRUTH[nm] = (g["hi"][off[nm]:off[nm] + n], g["lo"][off[nm]:off[nm] + n])
    return _TRUTH[name]


def regular(name):
    """The cases held to the bound: a value is defined (nr >= 1) and the case is not of the degenerate class."""
    return ~np.isnan(truth(name)[0]) & ~family(name)["degenerate"]


def _work(task):
    name, j = task
    return split(truth_mp(*args(family(name)), cases=[j])[0])


def write():
    """Compute every truth (one process per CPU) and write the fixture: a stored zip with fixed timestamps, so that the same truths
    give the same bytes."""
    import multiprocessing
    tasks = [(name, j) for name in names() for j in range(len(family(name)["nk"]))]
    with multiprocessing.Pool(os.cpu_count()) as pool:
        res = pool.map(_work, tasks, chunksize=4)
    arrays = dict(hi=np.array([r[0] for r in res]), lo=np.array([r[1] for r in res]), digest=digest())
    with zipfile.ZipFile(FIXTURE, "w", zipfile.ZIP_STORED) as z:
        for key, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, a, version=(1, 0))
            z.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())
    print("wrote %s: %d cases, %d bytes" % (FIXTURE, len(res), os.path.getsize(FIXTURE)))


if __name__ == "__main__":
    if sys.argv[1:] == ["--write"]:
        write()
    else:
        sys.exit("usage: python tests/_conds_ref.py --write")
