"""Reference statements for the implicit solves (wlsqm.hip.StencilSolver, csrc/krylov.hip), numpy only: the BiCGSTAB
recurrence as the kernels state it, on a dense matrix, and the builders of the systems that the tests solve.

The systems (SYSTEMS): on n uniformly random points of the unit square or cube, K nearest neighbours, order 2, the function value known
(b_F), centre weighting, h = n^(-1/dim):
  diffusion   I - tau h^2 Lap_h                                          (diag 1, scale -tau h^2, rows: the Laplacian)
  dirichlet   -Lap_h inside, identity rows within 1.2 h of the boundary  (diag 0, scale 1, per-case rows: e_F on the band)
and a diagonally dominant random structure (_stencil_ref.random_structure), not a fit.  Each names its `maxiter`: twice the iteration
count of bicgstab_ref on it (Jacobi, zero start, rtol 1e-10), which tests/test_krylov_host.py measures on the oracle's coefficients and
holds the constant to."""
import numpy as np

import _stencil_ref as R

RUNNING, CONVERGED, MAXITER, BREAKDOWN, NONFINITE, DIAGONAL = -1, 0, 1, 2, 3, 4
RTOL = 1e-10

# name: (kind, dim, K, n, tau, maxiter)
SYSTEMS = {
    "2D-tau0.25-n1000": ("diffusion", 2, 24, 1000, 0.25, 26),
    "2D-tau0.25-n130": ("diffusion", 2, 24, 130, 0.25, 18),
    "2D-tau1-n1000": ("diffusion", 2, 24, 1000, 1.0, 766),
    "2D-tau1-n130": ("diffusion", 2, 24, 130, 1.0, 122),
    "3D-tau0.25-n1000": ("diffusion", 3, 40, 1000, 0.25, 46),
    "2D-dirichlet-n1000": ("dirichlet", 2, 24, 1000, None, 130),
    "2D-dirichlet-n130": ("dirichlet", 2, 24, 130, None, 42),
    "3D-dirichlet-n1000": ("dirichlet", 3, 40, 1000, None, 40),
    "random-n130": ("random", 0, 9, 130, None, 16),
    "random-n1000": ("random", 0, 9, 1000, None, 16),
}


# What the GPU tests solve: all but I - h^2 Lap_h at n = 1000.  With the project's coefficients its one-sided boundary rows cost the matrix
# its positive diagonal (kappa_2 418 where the rehearsal with other weights had 32) and BiCGSTAB takes 383 erratic iterations: an iteration
# count and a residual gap that another summation order moves freely are no yardstick.  The host test keeps it as a record.
GPU_SYSTEMS = [name for name in SYSTEMS if name != "2D-tau1-n1000"]


# The first system twice more: from the start guess(n) with Jacobi, and from zero without a preconditioner; the caps as above.
FIRST = "2D-tau0.25-n1000"
VARIANTS = {"guess": 26, "plain": 22}


def guess(n):
    return np.random.default_rng([43, n]).standard_normal(n)


def square_structure(nrows, K, seed):
    """_stencil_ref.random_structure with npoints = nrows and row j naming point j (one full row with its own entry for nrows = 1, which
    random_structure does not make)."""
    if nrows == 1:
        rng = np.random.default_rng([seed, 1, K])
        return dict(hoods=np.zeros((1, K), np.int32), nk=np.full(1, K, np.int32), slots=rng.standard_normal((1, 1, K)),
                    own=rng.standard_normal((1, 1)), own_mask=np.ones(1, bool), pts=np.zeros(1, np.int32), npoints=1)
    st = R.random_structure(nrows, nrows, K, 1, seed=seed)
    st["pts"] = np.arange(nrows, dtype=np.int32)
    return st


def exact_dot(a, b):
    """(sum a_i b_i, sum |a_i b_i|) of two finite float arrays as Fractions, in integer arithmetic: _stencil_ref.exact_dot for long vectors."""
    from fractions import Fraction
    ma, ea = np.frexp(np.ravel(np.asarray(a, np.float64)))
    mb, eb = np.frexp(np.ravel(np.asarray(b, np.float64)))
    ia, ib = np.ldexp(ma, 53).astype(np.int64).tolist(), np.ldexp(mb, 53).astype(np.int64).tolist()
    e = (ea.astype(np.int64) + eb.astype(np.int64) - 106).tolist()
    emin = min(e) if e else 0
    total = mag = 0
    for x, y, k in zip(ia, ib, e):
        t = (x * y) << (k - emin)
        total += t
        mag += abs(t)
    two = Fraction(2) ** emin
    return total * two, mag * two


def maxiter(name):
    return SYSTEMS[name][5]


def jacobi(M):
    """1 / diag(M); inf or 0 where the diagonal is unusable (bicgstab_ref answers DIAGONAL)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return 1.0 / np.diag(M)


def bicgstab_ref(M, b, x0, dinv, rtol, atol, maxiter):
    """(x, iterations, status, history): right-preconditioned BiCGSTAB as csrc/krylov.hip runs it, dinv the inverse diagonal or None.
    history[k] is the recursive ||r||_2 after k iterations.  The status codes are the kernels'."""
    x = np.array(x0, np.float64)
    hist = []
    if dinv is not None and not (np.all(np.isfinite(dinv)) and np.all(dinv != 0.0)):
        return x, 0, DIAGONAL, hist
    pre = (lambda z: z) if dinv is None else (lambda z: dinv * z)
    with np.errstate(all="ignore"):
        r = b - M @ x
        r0 = r.copy()
        rr, bb = float(r @ r), float(b @ b)
        rho = rr
        if not (np.isfinite(rr) and np.isfinite(bb)):
            return x, 0, NONFINITE, hist
        stop = max(rtol * np.sqrt(bb), atol)
        hist.append(np.sqrt(rr))
        if np.sqrt(rr) <= stop:
            return x, 0, CONVERGED, hist
        if maxiter <= 0:
            return x, 0, MAXITER, hist
        rho_old = alpha = omega = 1.0
        p = v = None
        it = 0
        while True:
            p = r.copy() if it == 0 else r + (rho / rho_old) * (alpha / omega) * (p - omega * v)
            ph = pre(p)
            v = M @ ph
            den = float(r0 @ v)
            if not np.isfinite(den):
                return x, it, NONFINITE, hist
            if den == 0.0:
                return x, it, BREAKDOWN, hist
            alpha = rho / den
            if not np.isfinite(alpha):
                return x, it, NONFINITE, hist
            s = r - alpha * v
            sh = pre(s)
            t = M @ sh
            ts, tt = float(t @ s), float(t @ t)
            if not (np.isfinite(ts) and np.isfinite(tt)):
                return x, it, NONFINITE, hist
            omega = 0.0 if tt == 0.0 else ts / tt
            if not np.isfinite(omega):
                return x, it, NONFINITE, hist
            x = x + (alpha * ph + omega * sh)
            r = s - omega * t
            rho_old, rho, rr = rho, float(r0 @ r), float(r @ r)
            it += 1
            if not (np.isfinite(rho) and np.isfinite(rr)):
                return x, it, NONFINITE, hist
            hist.append(np.sqrt(rr))
            if np.sqrt(rr) <= stop:
                return x, it, CONVERGED, hist
            if it >= maxiter:
                return x, it, MAXITER, hist
            if rho == 0.0:
                return x, it, BREAKDOWN, hist
            if not np.isfinite((rho / rho_old) * (alpha / omega)):
                return x, it, NONFINITE, hist


def cloud(dim, n, K, seed=0):
    """(S (n, dim), hoods (n, K) int32: the K nearest other points of each, band (n,) bool: within 1.2 h of the boundary)."""
    rng = np.random.default_rng([17, dim, n, K, seed])
    S = rng.random((n, dim))
    d2 = ((S[:, None, :] - S[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d2, np.inf)
    hoods = np.argsort(d2, axis=1, kind="stable")[:, :K].astype(np.int32)
    h = n ** (-1.0 / dim)
    band = np.minimum(S, 1.0 - S).min(axis=1) < 1.2 * h
    return S, hoods, band


def laplacian_row(dim):
    """The Laplacian over the order-2 DOFs of wlsqm.fitter.defs."""
    import wlsqm
    no = {2: 6, 3: 10}[dim]
    row = np.zeros(no)
    for a in "XYZ"[:dim]:
        row[getattr(wlsqm, "i%d_%s2" % (dim, a))] = 1.0
    return row


def system(name):
    """What a test needs to build the system `name` on either side.  A fit: dict(kind, dim, order, S, hoods, nk, knowns, wm, rows
    (1, no) or (1, n, no), diag, scale, b, n).  The random structure: dict(kind, st (random_structure's, point j named by row j), diag
    (n,), scale, b, n)."""
    kind, dim, K, n, tau, _ = SYSTEMS[name]
    rng = np.random.default_rng([23, n, K])
    b = rng.standard_normal(n)
    if kind == "random":
        st = R.random_structure(n, n, K, 1, seed=29)
        st["pts"] = np.arange(n, dtype=np.int32)
        rows = R.rows_of(st["hoods"], st["nk"], st["slots"], st["own"], st["own_mask"], st["pts"])
        scale = -0.75
        diag = 1.0 + 1.5 * abs(scale) * np.array([sum(abs(v[0]) for _, v in r) for r in rows])
        return dict(kind=kind, st=st, diag=diag, scale=scale, b=b, n=n)
    import wlsqm
    S, hoods, band = cloud(dim, n, K)
    lap = laplacian_row(dim)
    h = n ** (-1.0 / dim)
    if kind == "diffusion":
        rows, diag, scale = lap[None, :].copy(), 1.0, -tau * h * h
    else:
        rows = np.where(band[:, None], np.eye(len(lap))[0][None, :], -lap[None, :])[None].copy()
        diag, scale = 0.0, 1.0
    return dict(kind=kind, dim=dim, order=2, S=S, hoods=hoods, nk=np.full(n, K, np.int32), knowns=np.full(n, 1, np.int64),
                wm=np.full(n, wlsqm.WEIGHT_CENTER, np.int32), rows=rows, diag=diag, scale=scale, b=b, n=n, band=band)


def dense_of(sy, A=None):
    """M = diag(d) + scale A dense.  A: the operator's plane as a dense array (the GPU tests pass the library's own); default: from the
    random structure, or for a fit from the CPU oracle's coefficients (its sensitivities contracted with the rows: _adjoint_ref)."""
    n = sy["n"]
    if A is None:
        if sy["kind"] == "random":
            st = sy["st"]
            A = R.dense(R.rows_of(st["hoods"], st["nk"], st["slots"], st["own"], st["own_mask"], st["pts"]), n, 0)
        else:
            import _adjoint_ref as AD
            g = np.ascontiguousarray(np.broadcast_to(sy["rows"][0], (n, sy["rows"].shape[-1])))
            ref = AD.adjoint_ref(sy["dim"], sy["order"], np.ascontiguousarray(sy["S"][sy["hoods"]]), sy["nk"], sy["S"], sy["knowns"], sy["wm"], g)
            rows = R.rows_of(sy["hoods"], sy["nk"], ref["grad_fk"][None], ref["grad_fi"][None, :, 0], np.ones(n, bool), np.arange(n))
            A = R.dense(rows, n, 0)
    d = sy["diag"] if np.ndim(sy["diag"]) else np.full(n, float(sy["diag"]))
    return np.diag(d) + sy["scale"] * A
