"""Reference statements for the block-Jacobi preconditioner over points of the coupled solves (wlsqm.hip.PointBlockJacobi,
csrc/krylov.hip), numpy only, on tests/_krylov_system_ref.py, _krylov_system_point_ref.py and _krylov_block_ref.py.

P = blockdiag(M_BB)^-1.  Block B holds the unknowns (i, a) of the points B points <= i < (B + 1) points, all a, in the interleaved
numbering i m + a: R = m points consecutive rows of the flat vectors, the last block cut at n and completed by the identity.

The entries of a block, stated once (block_statement) for both kinds of table, c the constant table or the point's own c[a, b, o, i]:
    entry ((i, a), (j, b)) = D_ab,i delta_ij + s,   s = the plain sum, from 0.0, over the stored entries e of row i with column j in
    entry order of t_ab(e) = c[a, b, 0] * val_0, then t = fma(c[a, b, o], val_o, t) for o = 1 .. nop - 1
The inverse is _krylov_block_ref.gauss_jordan_statement on the block padded by the identity to NB = the smallest of 8, 16, 32 that
holds R (pad_blocks).

The layout of the plane (layout, blocks_of_plane): a wave holds G = 64 / NB blocks, lane g NB + l is row l of block wave G + g, flat
row (wave G + g) R + l, live when l < R and the row is below m n; W[(wave NB + j) 64 + lane] is entry (l, j) of that block's inverse.

CAPS[(name, points, transposed)] is the `maxiter` of the GPU tests: twice the count of _krylov_block_ref.bicgstab_block_ref with numpy's
exact block inverses (zero start, rtol 1e-10) on the oracle's coefficients, which tests/test_krylov_system_block_host.py measures and
holds the constant to.  HOST_ONLY: the keys whose count the reversed summation order (same partition) moves by 1.25x or more."""
from fractions import Fraction

import numpy as np

import _krylov_block_ref as KB
import _krylov_ref as KR
import _krylov_system_point_ref as SP
import _krylov_system_ref as SR

EPS = 2.0 ** -53
fma = SR.fma


def default_points(m):
    """points=None: the largest value with m points <= 16."""
    return 16 // m


def nb_of(rows):
    return 8 if rows <= 8 else 16 if rows <= 16 else 32


# The systems: the names of _krylov_system_ref.SYSTEMS, and "point-" + name for a per-point table — the heterogeneous elasticity
# system of _krylov_system_point_ref, or a random structure whose table is scaled per point by 1 + 0.3 u, u uniform in (-1, 1) (the
# diagonal dominance of the random systems has a margin of 1.5).
# (name, points, transposed): maxiter, twice the reference's count (tests/test_krylov_system_block_host.py)
CAPS = {
    ("elasticity-2D-n130", 4, False): 74,
    ("elasticity-2D-n130", 8, False): 66,
    ("elasticity-2D-n130", 16, False): 50,
    ("elasticity-2D-n1000", 8, False): 192,
    ("elasticity-2D-n1000", 16, False): 168,
    ("elasticity-3D-n1000", 5, False): 86,
    ("elasticity-3D-n1000", 10, False): 78,
    ("reaction-2D-n130", 8, False): 16,
    ("random-m1", 16, False): 14,
    ("random-m2", 8, False): 16,
    ("random-m3", 5, False): 14,
    ("random-m4", 4, False): 14,
    ("elasticity-2D-n130", 8, True): 70,
    ("elasticity-3D-n1000", 5, True): 72,
    ("point-elasticity-2D-n130", 8, False): 64,
    ("point-elasticity-2D-n130", 8, True): 58,
    ("point-random-m3", 5, False): 14,
    ("point-random-m3", 5, True): 14,
}
HOST_ONLY = []
GPU_CASES = [key for key in CAPS if key not in HOST_ONLY]

# The gain: (name, points) whose count is compared with the Jacobi count of the same system, as the reference measures both.
GAIN = [("elasticity-2D-n1000", 8)]

_systems = {}


def system(name):
    """_krylov_system_ref.system's dict; "point-" + name: with `coupling` a per-point table (m, m, nop, n).  Computed once."""
    if name in _systems:
        return _systems[name]
    if not name.startswith("point-"):
        sy = SR.system(name)
    elif name == "point-random-m3":
        sy = dict(SR.system("random-m3"))
        u = np.random.default_rng([83, sy["n"]]).uniform(-1.0, 1.0, sy["n"])
        sy["coupling"] = SP.constant_table(sy["coupling"], sy["n"]) * (1.0 + 0.3 * u)
    else:
        sy = SP.system(name[len("point-"):])
    _systems[name] = sy
    return sy


def dense_matrix(A, coupling, diag):
    """The dense M of either kind of table from the dense planes A (nop, n, n)."""
    return (SP.dense_matrix if np.ndim(coupling) == 4 else SR.dense_matrix)(A, coupling, diag)


def dense_of(sy, A=None):
    return dense_matrix(SR.oracle_planes(sy) if A is None else A, sy["coupling"], sy["diag"])


def point_blocks_of(M, m, points):
    """(nblocks, R, R), R = m points: the diagonal blocks of the dense M over `points` points, the last one cut and completed by the
    identity."""
    return KB.blocks_of(M, m * points)


def pad_blocks(blocks, nb=None):
    """(nblocks, NB, NB): the blocks completed by the identity to NB rows (default: nb_of(R))."""
    nblocks, rows, _ = blocks.shape
    nb = nb_of(rows) if nb is None else nb
    out = np.tile(np.eye(nb), (nblocks, 1, 1))
    out[:, :rows, :rows] = blocks
    return out


def _coefficient(coupling, a, b, o, i):
    return coupling[a, b, o, i] if coupling.ndim == 4 else coupling[a, b, o]


def block_statement(rows, coupling, diag, points):
    """(nblocks, R, R): the blocks in the stated order of operations, every fma rounded once; the cut last block completed by the
    identity."""
    coupling = np.asarray(coupling, np.float64)
    m, nop, n = coupling.shape[0], coupling.shape[2], len(rows)
    D = SR.diag_blocks(diag, m, n)
    R_ = m * points
    nblocks = (n + points - 1) // points
    out = np.tile(np.eye(R_), (nblocks, 1, 1))
    for i, row in enumerate(rows):
        B = i // points
        first = B * points
        for a in range(m):
            s = np.zeros(R_)
            for c, v in row:
                if first <= c < first + points:
                    for b in range(m):
                        t = _coefficient(coupling, a, b, 0, i) * v[0]
                        for o in range(1, nop):
                            t = fma(_coefficient(coupling, a, b, o, i), v[o], t)
                        s[(c - first) * m + b] += t
            d = np.zeros(R_)
            d[(i - first) * m:(i - first) * m + m] = D[a, :, i]
            out[B, (i - first) * m + a] = d + s
    return out


def exact_blocks(rows, coupling, diag, points):
    """(exact, mag) (nblocks, R, R): the entries of the dense statement in exact arithmetic, rounded once, and the sums of the
    magnitudes of their terms c val and D; the identity where the cut last block is completed."""
    coupling = np.asarray(coupling, np.float64)
    m, nop, n = coupling.shape[0], coupling.shape[2], len(rows)
    D = SR.diag_blocks(diag, m, n)
    R_ = m * points
    nblocks = (n + points - 1) // points
    exact, mag = np.tile(np.eye(R_), (nblocks, 1, 1)), np.tile(np.eye(R_), (nblocks, 1, 1))
    F = lambda v: Fraction(float(v))
    for i, row in enumerate(rows):
        B = i // points
        first = B * points
        for a in range(m):
            for j in range(first, min(first + points, n)):
                for b in range(m):
                    terms = [F(_coefficient(coupling, a, b, o, i)) * F(v[o]) for c, v in row if c == j for o in range(nop)]
                    if i == j:
                        terms.append(F(D[a, b, i]))
                    at = (B, (i - first) * m + a, (j - first) * m + b)
                    exact[at] = float(sum(terms, Fraction(0)))
                    mag[at] = float(sum((abs(t) for t in terms), Fraction(0)))
    return exact, mag


def layout(n, m, points):
    """dict(nb, per, nblocks, nwaves, row): `row` (nwaves * 64,) is the flat row of every lane of the plane's waves, -1 where the lane is
    not live."""
    rows = m * points
    nb = nb_of(rows)
    per = 64 // nb
    nblocks = (n + points - 1) // points
    nwaves = (nblocks + per - 1) // per
    lane = np.arange(nwaves * 64) % 64
    wave = np.arange(nwaves * 64) // 64
    l = lane % nb
    row = (wave * per + lane // nb) * rows + l
    return dict(nb=nb, per=per, nblocks=nblocks, nwaves=nwaves, row=np.where((l < rows) & (row < m * n), row, -1),
                doubles=nwaves * nb * 64 + (nwaves + 3) // 4)


def blocks_of_plane(plane, n, m, points):
    """(nwaves * per, NB, NB): every block of a plane as the layout stores it, the blocks behind the last one and the padding included."""
    lay = layout(n, m, points)
    nb, per, nwaves = lay["nb"], lay["per"], lay["nwaves"]
    W = np.asarray(plane)[:nwaves * nb * 64].reshape(nwaves, nb, per, nb)            # [wave, j, g, l]
    return np.ascontiguousarray(np.transpose(W, (0, 2, 3, 1)).reshape(nwaves * per, nb, nb))


def apply_blocks(inv, v, transpose=False):
    """z (n, m) = blockdiag(inv) v on (n, m) vectors; inv (nblocks, R, R)."""
    return KB.apply_blocks(inv, np.asarray(v).reshape(-1), transpose).reshape(np.shape(v))


def mp_block_solves(blocks, v, dps=60):
    """(z, zt): blockdiag(blocks)^-1 v and blockdiag(blocks)^-T v in mpmath at `dps` digits, rounded to float64 —
    _krylov_block_ref.mp_block_solve for a matrix and its transpose from one LU decomposition per block (P B = L U, so
    B^T = U^T L^T P: a forward substitution with U^T, a backward one with L^T, and the row exchanges undone in reverse order)."""
    import mpmath
    nblocks, nb, _ = blocks.shape
    full = np.zeros(nblocks * nb)
    full[:len(v)] = v
    out, out_t = np.zeros(nblocks * nb), np.zeros(nblocks * nb)
    with mpmath.workdps(dps):
        mp = mpmath.mp
        for B in range(nblocks):
            rhs = full[B * nb:B * nb + nb].tolist()
            LU, p = mp.LU_decomp(mpmath.matrix(blocks[B].tolist()))
            z = mp.U_solve(LU, mp.L_solve(LU, mpmath.matrix(rhs), p))
            out[B * nb:B * nb + nb] = [float(t) for t in z]
            y = [mpmath.mpf(t) for t in rhs]
            for i in range(nb):                                          # U^T y = v
                for k in range(i):
                    y[i] -= LU[k, i] * y[k]
                y[i] /= LU[i, i]
            for i in range(nb - 1, -1, -1):                              # L^T w = y, the unit diagonal
                for k in range(i + 1, nb):
                    y[i] -= LU[k, i] * y[k]
            for k in range(len(p) - 1, -1, -1):                          # z = P^T w
                y[k], y[p[k]] = y[p[k]], y[k]
            out_t[B * nb:B * nb + nb] = [float(t) for t in y]
    return out[:len(v)], out_t[:len(v)]


def preconditioner(M, m, points):
    """The callable of _krylov_block_ref.bicgstab_block_ref: numpy's exact inverses of point_blocks_of(M, m, points).  For M^T pass
    M^T: its blocks are the transposes."""
    inv = np.linalg.inv(point_blocks_of(M, m, points))
    return lambda z: KB.apply_blocks(inv, z)


def solve_ref(M, b, m, points, x0=None, cap=5000, reverse=False):
    """bicgstab_block_ref at rtol 1e-10 on flat b; reverse: on the system with rows and columns reversed — another summation order —
    under the same partition into blocks (the preconditioner is applied in the matrix's own numbering), x returned in that numbering."""
    pre = preconditioner(M, m, points)
    x0 = np.zeros(len(b)) if x0 is None else x0
    if reverse:
        Mr = np.ascontiguousarray(M[::-1, ::-1])
        x, its, status, hist = KB.bicgstab_block_ref(Mr, b[::-1].copy(), x0[::-1].copy(), lambda z: pre(z[::-1])[::-1], KR.RTOL, 0.0, cap)
        return x[::-1], its, status, hist
    return KB.bicgstab_block_ref(M, b, x0, pre, KR.RTOL, 0.0, cap)


def matrix_of(key, A=None):
    """(sy, M, b flat) of a key of CAPS: M is the transposed matrix for a transposed key."""
    name, points, transposed = key
    sy = system(name)
    M = dense_of(sy, A)
    return sy, (np.ascontiguousarray(M.T) if transposed else M), sy["b"].reshape(-1)


def singular_point_system(n=64):
    """dict(st, coupling, diag, b): m = 2 on a structure of one plane whose point 0 has the own 2 x 2 block [[1, 1], [1, 1]] — singular,
    with a non-zero diagonal — inside a regular M: coupling[a, a] = 1 and coupling[0, 1] = coupling[1, 0] = c, D = d I, and point 0
    carries the own entry w with d + w = 1 and c w = 1 (w = -2, d = 3, c = -0.5).  Every other point is diagonally dominant: 3 on the
    diagonal, 0.1 (times 1 or c) beside it, except that points 0 and 1 name each other with 0.5 and 1.  The scalar diagonal is 1 at point 0 and 3 elsewhere, so Jacobi goes through."""
    i = np.arange(n)
    hoods = np.stack([(i + 1) % n, (i + 5) % n], axis=1).astype(np.int32)
    slots = np.full((1, n, 2), 0.1)
    own, own_mask = np.zeros((1, n)), np.zeros(n, bool)
    own[0, 0], own_mask[0] = -2.0, True
    hoods[0], slots[0, 0] = (1, 5), (0.5, 0.1)                          # points 0 and 1 name each other with entries of size 1:
    hoods[1], slots[0, 1] = (0, 6), (1.0, 0.1)                          # the Schur complement of point 0 is regular
    st = dict(hoods=hoods, nk=np.full(n, 2, np.int32), slots=slots, own=own, own_mask=own_mask, pts=i.astype(np.int32), npoints=n)
    coupling = np.array([[[1.0], [-0.5]], [[-0.5], [1.0]]])
    b = np.random.default_rng([89, n]).standard_normal((n, 2))
    return dict(st=st, coupling=coupling, diag=3.0, b=b, m=2, nop=1, n=n)


# The worst _krylov_block_ref.worst_ratio (unit: NB eps kappa_inf(B) |z|_inf) of gauss_jordan_statement on the padded blocks against
# mp_block_solve, over the (system, points) of STATEMENT_ON and the square structures that the GPU test takes, as
# tests/test_krylov_system_block_host.py measures it (0.34 when the constant was set) and holds this constant to: measured <= STATEMENT_RATIO <= 2 measured.  The GPU
# bound is 4 times this: the margin for fma and for the order in which the kernel's lanes take the pivot row.
STATEMENT_ON = (("elasticity-2D-n1000", 8), ("elasticity-3D-n1000", 5), ("elasticity-2D-n130", 4), ("random-m4", 4))
STATEMENT_RATIO = 0.5

# The square structures of the GPU test of the blocks: planes_structure(n, 9, RANDOM_NOP[m], seed) with these sizes and points.
BLOCK_SIZES = (1, 15, 16, 17, 63, 64, 65, 130, 300)
BLOCK_POINTS = {1: (8, 16, 32), 2: (1, 3, 4, 7, 8, 16), 3: (1, 2, 5, 10), 4: (2, 3, 4, 8)}
BLOCK_SEED = 97


def block_cases(m=None, points=None):
    """[(m, n, points, form, point)]: every size with every points of every m (or of the given ones), the three forms of diag and the
    two kinds of table taken in turn."""
    out = []
    for mm, pts in BLOCK_POINTS.items():
        for k, p in enumerate(pts):
            for j, n in enumerate(BLOCK_SIZES):
                if (m is None or m == mm) and (points is None or points == p):
                    out.append((mm, n, p, ("float", "constants", "tensor")[(k + j) % 3], bool(((k + j) // 3 + mm) % 2)))
    return out


def gain_ratio(M, b, m, points):
    """The blocks' iteration count over Jacobi's, both by the reference on the same matrix (zero start, rtol 1e-10)."""
    its, status = solve_ref(M, b, m, points)[1:3]
    jac, jstatus = SR.solve_ref(M, b, "jacobi")[1:3]
    assert status == jstatus == KR.CONVERGED
    return its / jac


def block_case(n, m, form, point):
    """(st, rows, coupling, diag) of one case of the GPU test of the blocks: a random square structure with 3 m nop on the diagonal of D, which
    keeps the blocks away from singular without making them diagonal.  form: "float", "constants" or "tensor" (diag); point: a per-point table."""
    nop = SR.RANDOM_NOP[m]
    st = SR.planes_structure(n, 9, nop, seed=BLOCK_SEED)
    rows = SR.rows_of_structure(st)
    rng = np.random.default_rng([BLOCK_SEED, n, m, int(point)])
    coupling = rng.standard_normal((m, m, nop, n) if point else (m, m, nop))
    size = 3.0 * m * nop
    if form == "float":
        diag = size
    elif form == "constants":
        diag = rng.standard_normal((m, m)) + size * np.eye(m)
    else:
        diag = rng.standard_normal((m, m, n)) + size * np.eye(m)[:, :, None]
    return st, rows, coupling, diag
