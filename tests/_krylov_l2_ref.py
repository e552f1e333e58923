"""Reference statements for BiCGSTAB(2) (wlsqm.hip.StencilSolver(method="bicgstab2"), csrc/krylov.hip), numpy only:
the recurrence as the kernels state it, on a dense matrix with a callable preconditioner, and the 3D systems at tau = 1 that the method is
for.  Every other system is tests/_krylov_block_ref.morton_system's.

The recurrence, right-preconditioned (A = M P), rt the residual of the start:

  start:  r = rt = b - M x;  rho0 = 1, alpha = 0, omega = 1;  the threshold and the immediate stop of tests/_krylov_ref.bicgstab_ref
  cycle:  rho0 = -omega rho0
    j = 0:  rho1 = (rt, r);  beta = alpha rho1 / rho0;  rho0 = rho1;  u = r - beta u (the first cycle: u = r);  u1 = A u
            alpha = rho0 / (rt, u1);  r = r - alpha u1;  r1 = A r;  dy = alpha u
    j = 1:  rho1 = (rt, r1); beta = alpha rho1 / rho0;  rho0 = rho1;  u = r - beta u, u1 = r1 - beta u1;  u2 = A u1
            alpha = rho0 / (rt, u2);  r = r - alpha u1, r1 = r1 - alpha u2;  r2 = A r1;  dy += alpha u
    MR:     s1 = (r1, r1), c1 = (r, r1), a12 = (r2, r1), a22 = (r2, r2), c2 = (r, r2)
            tau = a12 / s1;  s2 = a22 - tau a12;  g2 = (c2 - tau c1) / s2;  g1 = c1 / s1 - tau g2;  omega = g2
            x += P (dy + g1 r + g2 r1);  r = r - g1 r1 - g2 r2;  u = u - g1 u1 - g2 u2
            (rt, r) and (r, r);  iterations += 2;  the stop test

(rt, u1) == 0 stops at once with status 2.  (rt, u2) == 0 finds the cycle holding the step j = 0, which x has not received: it takes
alpha = 0 and rho0 = 0, the cycle ends as ever (x takes alpha_0 u_0 and the minimisation, r stays b - M x), and the next cycle's head
answers status 2 unless that converged: the rule of omega = 0.  A system of one row always ends here, since its Krylov space has one
dimension: either r vanishes at j = 0 (then u1 = u2 = 0) or the new direction u1 does.

`iterations` and `maxiter` count pairs of products: a cycle adds 2, and the stop, the limit and the breakdown of the next cycle's head are
taken at the end of a cycle.  x is written once per cycle, behind every check of the cycle's scalars.

CAPS[name][precond] is the `maxiter` of the GPU tests: twice the iteration count of bicgstab2_ref on that system (zero start, rtol 1e-10),
which tests/test_krylov_l2_host.py measures on the oracle's coefficients and holds the constant to.  precond: None, "jacobi" or a block
size."""
import numpy as np

import _krylov_block_ref as KB
import _krylov_ref as KR

# name: (dim, K, n, tau): I - tau h^2 Lap_h, order 2, on a cloud in Morton order
SYSTEMS_3D = {
    "3D-tau1-n130": (3, 40, 130, 1.0),
    "3D-tau1-n1000": (3, 40, 1000, 1.0),
    "3D-tau1-n2000": (3, 40, 2000, 1.0),
}


def system(name):
    """tests/_krylov_block_ref.morton_system(name), or one of SYSTEMS_3D built the same way: tests/_krylov_ref.cloud's points in Morton
    order, the K nearest neighbours found on the sorted table, the right-hand side of tests/_krylov_ref.system."""
    if name not in SYSTEMS_3D:
        return KB.morton_system(name)
    import synth
    import wlsqm
    dim, K, n, tau = SYSTEMS_3D[name]
    b = np.random.default_rng([23, n, K]).standard_normal(n)
    S = KR.cloud(dim, n, K)[0]
    S = np.ascontiguousarray(S[synth.morton_order(S)])
    d2 = ((S[:, None, :] - S[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d2, np.inf)
    hoods = np.argsort(d2, axis=1, kind="stable")[:, :K].astype(np.int32)
    h = n ** (-1.0 / dim)
    band = np.minimum(S, 1.0 - S).min(axis=1) < 1.2 * h
    return dict(kind="diffusion", dim=dim, order=2, S=S, hoods=hoods, nk=np.full(n, K, np.int32), knowns=np.full(n, 1, np.int64),
                wm=np.full(n, wlsqm.WEIGHT_CENTER, np.int32), rows=KR.laplacian_row(dim)[None, :].copy(), diag=1.0, scale=-tau * h * h,
                b=b, n=n, band=band)


def preconditioner(M, precond, reverse=False):
    """What bicgstab2_ref takes as `pre`: None, the inverse diagonal (an array: status 4 when it is unusable) or the callable of the
    block inverses.  reverse: for the system with rows and columns reversed (M is the matrix in its own order): the same blocks."""
    if precond is None:
        return None
    if precond == "jacobi":
        d = KR.jacobi(M)
        return d[::-1].copy() if reverse else d
    inv = KB.block_inverses(M, precond)
    if reverse:
        return lambda z: KB.apply_blocks(inv, z[::-1])[::-1]
    return lambda z: KB.apply_blocks(inv, z)


def minimise(s1, c1, a12, a22, c2):
    """(g1, g2) of min ||r - g1 r1 - g2 r2|| through the 2 x 2 normal equations, r1 eliminated first.  s1 == 0: both 0; s2 == 0 (r2 in
    the span of r1): g2 = 0 and g1 = c1 / s1."""
    g1 = g2 = 0.0
    if s1 != 0.0:
        tau = a12 / s1
        s2 = a22 - tau * a12
        if s2 != 0.0:
            g2 = (c2 - tau * c1) / s2
        g1 = c1 / s1 - tau * g2
    return g1, g2


def bicgstab2_ref(M, b, x0, pre, rtol, atol, maxiter):
    """(x, iterations, status, history): the recurrence of the module's docstring as csrc/krylov.hip runs it.  pre: None, a callable, or
    the inverse diagonal as an array.  history[k] is the recursive ||r||_2 after k cycles.  The status codes are the kernels'."""
    x = np.array(x0, np.float64)
    hist = []
    if isinstance(pre, np.ndarray):
        dinv = pre
        if not (np.all(np.isfinite(dinv)) and np.all(dinv != 0.0)):
            return x, 0, KR.DIAGONAL, hist
        pre = lambda z: dinv * z
    P = (lambda z: z) if pre is None else pre
    fin = np.isfinite
    with np.errstate(all="ignore"):
        r = b - M @ x
        rt = r.copy()
        rr, bb = float(r @ r), float(b @ b)
        if not (fin(rr) and fin(bb)):
            return x, 0, KR.NONFINITE, hist
        stop = max(rtol * np.sqrt(bb), atol)
        hist.append(np.sqrt(rr))
        if np.sqrt(rr) <= stop:
            return x, 0, KR.CONVERGED, hist
        if maxiter <= 0:
            return x, 0, KR.MAXITER, hist
        rho0, alpha, omega, rho1 = 1.0, 0.0, 1.0, rr
        u = u1 = None
        it = 0
        while True:
            rho0 = -omega * rho0
            if rho0 == 0.0:
                return x, it, KR.BREAKDOWN, hist
            beta = alpha * rho1 / rho0
            if not fin(beta):
                return x, it, KR.NONFINITE, hist
            rho0 = rho1
            # j = 0
            u = r.copy() if it == 0 else r - beta * u
            u1 = M @ P(u)
            den = float(rt @ u1)
            if not fin(den):
                return x, it, KR.NONFINITE, hist
            if den == 0.0:
                return x, it, KR.BREAKDOWN, hist
            alpha = rho0 / den
            if not fin(alpha):
                return x, it, KR.NONFINITE, hist
            r = r - alpha * u1
            dy = alpha * u
            r1 = M @ P(r)
            # j = 1
            rho1 = float(rt @ r1)
            if not fin(rho1):
                return x, it, KR.NONFINITE, hist
            if rho0 == 0.0:
                return x, it, KR.BREAKDOWN, hist
            beta = alpha * rho1 / rho0
            if not fin(beta):
                return x, it, KR.NONFINITE, hist
            rho0 = rho1
            u = r - beta * u
            u1 = r1 - beta * u1
            u2 = M @ P(u1)
            den = float(rt @ u2)
            if not fin(den):
                return x, it, KR.NONFINITE, hist
            if den == 0.0:                                               # the breakdown waits for the end of the cycle
                alpha, rho0 = 0.0, 0.0
            else:
                alpha = rho0 / den
            if not fin(alpha):
                return x, it, KR.NONFINITE, hist
            r = r - alpha * u1
            r1 = r1 - alpha * u2
            dy = dy + alpha * u
            r2 = M @ P(r1)
            # the minimisation of ||r - g1 r1 - g2 r2||
            s1, c1, a12, a22, c2 = float(r1 @ r1), float(r @ r1), float(r2 @ r1), float(r2 @ r2), float(r @ r2)
            if not (fin(s1) and fin(c1) and fin(a12) and fin(a22) and fin(c2)):
                return x, it, KR.NONFINITE, hist
            g1, g2 = minimise(s1, c1, a12, a22, c2)
            if not (fin(g1) and fin(g2)):
                return x, it, KR.NONFINITE, hist
            omega = g2
            x = x + P((dy + g1 * r) + g2 * r1)
            r, u = (r - g1 * r1) - g2 * r2, (u - g1 * u1) - g2 * u2
            rho1, rr = float(rt @ r), float(r @ r)
            it += 2
            if not (fin(rho1) and fin(rr)):
                return x, it, KR.NONFINITE, hist
            hist.append(np.sqrt(rr))
            if np.sqrt(rr) <= stop:
                return x, it, KR.CONVERGED, hist
            if it >= maxiter:
                return x, it, KR.MAXITER, hist


def solve_ref(M, b, precond, cap=20000, reverse=False):
    """The reference from zero at rtol 1e-10; reverse: on the system with rows and columns reversed (another summation order, the same
    blocks), x returned in the matrix's own order."""
    n = len(b)
    if reverse:
        x, its, status, hist = bicgstab2_ref(M[::-1, ::-1], b[::-1], np.zeros(n), preconditioner(M, precond, True), KR.RTOL, 0.0, cap)
        return x[::-1], its, status, hist
    return bicgstab2_ref(M, b, np.zeros(n), preconditioner(M, precond), KR.RTOL, 0.0, cap)


PRECONDS = (None, "jacobi", 16)

# name: {precond: maxiter}: what tests/test_gpu_krylov_l2.py solves.
CAPS = {
    "2D-tau0.25-n130": {None: 16, "jacobi": 16, 16: 12},
    "2D-tau1-n130": {None: 44, "jacobi": 76, 8: 28, 16: 24, 32: 20},      # n = 130 leaves a last block of 2 rows
    "2D-tau1-n1000": {None: 152, "jacobi": 296, 16: 72},
    "3D-tau0.25-n1000": {None: 28, "jacobi": 36, 16: 24},
    "2D-dirichlet-n1000": {None: 136, "jacobi": 144, 16: 92},
    "3D-tau1-n130": {None: 160, "jacobi": 380, 16: 144},
    "random-n130": {None: 44, "jacobi": 16, 16: 16},
}

# The two systems of the headline, blocks of 16 only: name: maxiter.  BiCGSTAB with the same blocks breaks down on the second.
HEADLINE = {"3D-tau1-n1000": 1772, "3D-tau1-n2000": 2672}

# The transposed solve of the GPU tests: (name, precond, maxiter), twice the reference's count on M^T with the transposed blocks.
TRANSPOSED = ("2D-dirichlet-n130", 16, 28)

# (name, precond) pairs whose count under the reversed summation order leaves 1.25x of the plain one: a count that the order of a sum
# moves that far is no yardstick for a device whose sums run in yet another order (tests/test_krylov_l2_host.py holds the rule).
HOST_ONLY = []
GPU_CASES = [(name, pc) for name, caps in CAPS.items() for pc in caps if (name, pc) not in HOST_ONLY]
