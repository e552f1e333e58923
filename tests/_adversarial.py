"""Structured and adversarial neighbourhoods for the fit kernels.

Every other input of the suite is drawn the same way (origins in [0, 1]^d, offsets uniform in a cube of half-width 0.05 or Halton
points, the field sin(3x) cos(2y)).  The families here are what users produce instead: lattices with exact distance ties, corner
points, stretched meshes, clouds far from the origin, kNN lists that contain the point itself, data with a large offset or at the
ends of the exponent range.  Each generator is deterministic (seeded by family, shape and n), takes (dim, order, K, n) and returns
one batch `dict(xk, fk, nk, xi, fi0, order, no, note)` in the layout of fit_*D_many (1D: xk (n, K), xi (n,)).  A family is a batch
of its own: its cases have similar conditioning, so a max-over-batch column metric means something.

No generator filters cases: every case it draws is in the batch.
"""
import zlib

import numpy as np

NDOF = {1: [1, 2, 3, 4, 5], 2: [1, 3, 6, 10, 15], 3: [1, 4, 10, 20, 35]}
H = 0.05                      # half-width of the plain neighbourhood
GRID_H = 2.0 ** -5            # lattice spacing (dyadic: node coordinates and offsets are exact)

# tiny / huge: the whole problem scaled by 10^-30 / 10^+30.  The oracle's result is finite on every case at every shape of SHAPES,
# order 4 included (its largest intermediate there is (0.05 * 10^+-30)^8 / 576, still a normal double), so no shape needs a smaller
# exponent (tests/test_adversarial_cpu.py asserts the finiteness).
SCALE_EXP = 30

# collinear: y = 0.7 x + eps * noise.  eps = 1e-2 gives kappa ~ 1e4 at order 2, but kappa grows like eps^-order: 1.4e7 at order 3 and
# 1e9 at order 4, where the oracle's own error against the truth is of order one (N = 4.8 in 2D, 31 in 3D: finite garbage: no reference).
# The noise is therefore widened with the order so that kappa stays near 1e4 and the oracle stays a reference.
# 3D order 4 has its own value: eps = 0.2 leaves kappa at 8.5e4 there (2D: 7e3), and at that conditioning a 16-case batch is a small sample
# for criterion (a) (the 2-lane emulation measured 1.2x its bound on one column, the 1- and 4-lane ones 0.4x); 0.35 brings kappa to 1e4.
COLLINEAR_EPS = {0: 1e-2, 1: 1e-2, 2: 1e-2, 3: 1e-1, 4: 2e-1, (3, 4): 0.35}

SHAPES = ((2, 2, 32), (2, 3, 30), (2, 4, 64), (3, 2, 40), (3, 3, 64), (3, 4, 64), (1, 2, 8), (1, 4, 12))

# tiny_edge / huge_edge: the same, at the largest power of ten per order at which the oracle is still finite on every case of a 256-case
# batch at every shape of that order (the next power of ten gives inf / NaN in the oracle at some shape): the products of two monomials of
# degree `order` then sit within a few decades of the ends of the exponent range, where a divide or square-root sequence that skips its range
# handling differs from the IEEE one.  (tiny / huge at 1e-+30 trip the range CHECKS of the accurate and strict kernels, 2^-+200, but are
# too far from the ends for the unguarded sequences to round differently.)  Order 2 / tiny is one decade short of the oracle's limit (1e-75):
# there the fast arithmetic's unscaled LDL^T overflows in 1D (a denormal pivot; the CPU emulation returns inf where the oracle's q is 90), which
# DESIGN section 2 records as the fast mode's narrower range; at 1e-74 the emulation is at 0.95x the oracle's q.
EDGE_EXP = {"tiny_edge": {2: 74, 3: 49, 4: 36}, "huge_edge": {2: 78, 3: 52, 4: 39}}

FAMILIES = ("plain", "grid", "grid_sorted", "sortedguess", "far", "aniso", "onesided", "self", "collinear", "tiny", "huge", "tiny_edge",
            "huge_edge", "fkoffset", "fkscale_lo", "fkscale_hi", "exactpoly", "exactpoly_grid")


def field(x):
    return np.sin(3 * x[..., 0]) * np.cos(2 * x[..., -1])


def _rng(family, dim, order, K, n):
    return np.random.default_rng([zlib.crc32(family.encode()), dim, order, K, n])


# ---- the regular lattice -----------------------------------------------------------------------------------------------------------

def lattice_shells(dim, count):
    """Integer offsets of a d-dimensional lattice, centre excluded, ascending by squared length: (offsets (m, dim), r2 (m,)) with
    every shell complete and m >= count."""
    R = 1
    while True:
        ax = np.arange(-R, R + 1)
        g = np.stack(np.meshgrid(*([ax] * dim), indexing="ij"), axis=-1).reshape(-1, dim)
        r2 = (g * g).sum(axis=1)
        keep = (r2 > 0) & (r2 <= R * R)                 # the ball inscribed in the cube holds complete shells only
        if keep.sum() >= count:
            g, r2 = g[keep], r2[keep]
            o = np.lexsort(tuple(g[:, m] for m in range(dim - 1, -1, -1)) + (r2,))
            return g[o], r2[o]
        R += 1


def shell_counts(dim, K):
    """(K_complete, K_cut): the largest neighbour count <= K that ends on a complete distance shell with at least two members, and
    the largest count <= K that takes at least two but not all members of its last shell (0 if there is none, as in 1D)."""
    _, r2 = lattice_shells(dim, K + 1)
    ends = np.nonzero(np.diff(r2))[0] + 1               # counts at which a shell is complete
    ends = ends[ends <= K]
    complete = int(ends[-1])
    cut = 0
    for c in range(K, 1, -1):
        start = int(ends[ends < c][-1]) if (ends < c).any() else 0
        if c not in ends and c - start >= 2:
            cut = c
            break
    return complete, cut


def grid_rows(dim, K, n, rng, guess=False):
    """Per case: an origin on the lattice and nk[j] <= K nearest nodes (centre excluded).  Cases cycle through four arrangements:
    complete last shell / sorted, complete / shuffled, last shell cut / sorted, cut / shuffled.  Which members of a cut shell are
    taken is drawn per case; the rows are sorted by distance (ties in lattice order) or shuffled as a whole.  Slots k >= nk[j] repeat
    the first neighbour (never read).  Cases 2i and 2i + 1 hold the same neighbourhood, sorted and shuffled.
    guess=True: no row is shuffled; the odd cases move their whole last shell to the FRONT of the row instead, so that the rest of the row
    still ascends (the last slots of every row of the batch are sorted) while the farthest neighbours sit in the first slots and the last
    neighbour is strictly nearer than they are.  The even cases end on their ties: the last neighbour IS at the largest distance."""
    offs, r2 = lattice_shells(dim, K + 1)
    complete, cut = shell_counts(dim, K)
    node = rng.integers(8, 24, (n, dim))
    node[1::2] = node[0:n - 1:2]                                   # cases 2i (sorted) and 2i + 1 (shuffled) are the same neighbourhood
    idx = np.zeros((n, K), np.int64)
    nk = np.zeros(n, np.int32)
    arrangement = np.arange(n) % 4
    for j in range(n):
        a = arrangement[j]
        c = complete if (a < 2 or not cut) else cut
        if a % 2 == 0:
            chosen = np.sort(np.lexsort((rng.random(len(r2)), r2))[:c])   # the c nearest, ties drawn; then ascending distance, ties in lattice order
        if guess and a % 2 == 1:
            last = r2[chosen] == r2[chosen[-1]]
            order_j = np.concatenate([chosen[last], chosen[~last]])
        else:
            order_j = chosen if a % 2 == 0 else rng.permutation(chosen)
        idx[j, :c] = order_j
        idx[j, c:] = order_j[0]
        nk[j] = c
    steps = offs[idx]                                              # (n, K, dim) integers
    xi = node * GRID_H
    xk = (node[:, None, :] + steps) * GRID_H
    return xi, xk, nk, arrangement, dict(node=node, steps=steps)


# ---- polynomials -------------------------------------------------------------------------------------------------------------------

def exponents(dim, order):
    import _parity as P
    return P.exponents(dim, order)


def poly_eval(dim, order, coef, d):
    """sum_a coef[..., a] * prod_m d_m^p / p! at offsets d (..., dim): the fit's own model, so `coef` IS the expected fi."""
    fact = [1.0, 1.0, 2.0, 6.0, 24.0]
    out = np.zeros(d.shape[:-1])
    for a, e in enumerate(exponents(dim, order)):
        term = np.ones(d.shape[:-1])
        for m, p in enumerate(e):
            if p:
                term = term * d[..., m] ** p / fact[p]
        out = out + coef[:, a, None] * term
    return out


# ---- the families ------------------------------------------------------------------------------------------------------------------

def make(family, dim, order, K, n):
    """One batch of `family`.  Keys: xk, fk, nk, xi, fi0 (random start values; column 0 holds the field at the origin, so that
    knowns = b?_F is a consistent problem), order, no, dim, K; `coef` for the polynomial fields (the exact answer); `arrangement`,
    `lattice` for the lattice families."""
    assert family in FAMILIES, family
    rng = _rng(family, dim, order, K, n)
    no = NDOF[dim][order]
    nk = np.full(n, K, np.int32)
    extra = {}
    xi = rng.uniform(0, 1, (n, dim))
    unit = rng.uniform(-1, 1, (n, K, dim))
    off = H * unit
    f_at = field
    fk = f0 = None
    if family in ("plain", "fkoffset", "fkscale_lo", "fkscale_hi", "tiny", "huge", "tiny_edge", "huge_edge", "exactpoly"):
        xk = xi[:, None, :] + off
    elif family == "sortedguess":
        # every row ascending by distance (a kNN search's rows); case 3i keeps it (the last neighbour is the farthest), case 3i + 1 has its
        # farthest neighbour moved to slot 0 and case 3i + 2 to slot K // 4: the rest still ascends, so the last slots of EVERY row are
        # sorted while in two rows of three a strictly farther neighbour sits early in the row
        xk = xi[:, None, :] + off
        d = xk - xi[:, None, :]
        o = np.argsort((d * d).sum(axis=-1), axis=1, kind="stable")
        for j in range(n):
            if j % 3:
                o[j] = np.insert(o[j, :-1], 0 if j % 3 == 1 else K // 4, o[j, -1])
        xk = np.take_along_axis(xk, o[:, :, None], axis=1)
    elif family == "far":
        xi = (xi + 1e6)
        xk = (xi[:, None, :] + off)
        f_at = lambda x: field(x - 1e6)                  # x - 1e6 is exact: the data belong to the rounded geometry
    elif family == "aniso":
        stretch = {1: (1.0,), 2: (1.0, 1e-3), 3: (1.0, 1e-2, 1e-3)}[dim]
        xk = xi[:, None, :] + off * np.array(stretch)
    elif family == "onesided":
        xk = xi[:, None, :] + H * np.abs(unit)
    elif family == "self":
        xk = xi[:, None, :] + off
        xk[:, 0, :] = xi
        xk[:, 2, :] = xk[:, 1, :]
    elif family == "collinear":
        noise = H * rng.uniform(-1, 1, (n, K, dim))
        o2 = off.copy()
        for m in range(1, dim):
            o2[..., m] = 0.7 * off[..., 0] + COLLINEAR_EPS.get((dim, order), COLLINEAR_EPS[order]) * noise[..., m]
        xk = xi[:, None, :] + o2
    elif family in ("grid", "grid_sorted", "exactpoly_grid"):
        xi, xk, nk, arr, lat = grid_rows(dim, K, n, rng, guess=family == "grid_sorted")
        extra.update(arrangement=arr, lattice=lat)
    if family in ("exactpoly", "exactpoly_grid"):
        if family == "exactpoly_grid":
            # dyadic, and a multiple of the monomial's factorials: every term c_a d^p / p! and their sum are exact on the lattice
            mult = np.array([np.prod([(1, 1, 2, 6, 24)[p] for p in e]) for e in exponents(dim, order)], float)
            coef = rng.integers(-64, 65, (n, no)) / 8.0 * mult
        else:
            coef = rng.uniform(-1, 1, (n, no)) / H ** np.array([sum(e) for e in exponents(dim, order)])   # every term of order one at H
        d = xk - xi[:, None, :]
        fk = poly_eval(dim, order, coef, d)
        f0 = coef[:, 0].copy()
        extra["coef"] = coef
    if fk is None:
        fk = f_at(xk)
        f0 = f_at(xi)
    if family == "fkoffset":
        fk = fk + 1e6; f0 = f0 + 1e6
    if family in ("fkscale_lo", "fkscale_hi"):
        s = 1e-150 if family == "fkscale_lo" else 1e150
        fk = fk * s; f0 = f0 * s
    if family in ("tiny", "huge", "tiny_edge", "huge_edge"):
        e = SCALE_EXP if family in ("tiny", "huge") else EDGE_EXP[family][max(order, 2)]
        s = 10.0 ** (-e if family.startswith("tiny") else e)
        xi = xi * s; xk = xk * s                                                 # the field stays on the unscaled coordinates
        extra["scale"] = s
    fi0 = rng.uniform(-1, 1, (n, no))
    fi0[:, 0] = f0
    if dim == 1:
        xk = np.ascontiguousarray(xk[..., 0]); xi = np.ascontiguousarray(xi[:, 0])
    out = dict(family=family, dim=dim, order=order, K=K, n=n, no=no, xk=np.ascontiguousarray(xk), fk=np.ascontiguousarray(fk), nk=nk,
               xi=np.ascontiguousarray(xi), fi0=fi0, order_a=np.full(n, order, np.int32))
    out.update(extra)
    return out


def point_table(b, rng=None):
    """The batch as an index-based problem: a point table S (origins first, then every neighbour slot), the data F on it, hoods into it
    and point_index.  Gathering S[hoods] gives back xk bit for bit."""
    n, K, dim = b["n"], b["K"], b["dim"]
    xi = b["xi"].reshape(n, -1); xk = b["xk"].reshape(n, K, -1)
    S = np.concatenate([xi, xk.reshape(n * K, -1)])
    F = np.concatenate([b["fi0"][:, 0], b["fk"].reshape(-1)])
    hoods = (n + np.arange(n * K).reshape(n, K)).astype(np.int32)
    pidx = np.arange(n, dtype=np.int32)
    if dim == 1:
        S = np.ascontiguousarray(S[:, 0])
    return S, F, hoods, pidx


def lattice_cloud(dim, K, f=field):
    """A real lattice of 32^2 / 16^3 / 512 (1D) nodes and, for every interior node far enough from the faces, its kNN list
    INCLUDING the node itself in slot 0 (what cKDTree(S).query(S, K) returns): ascending distance, ties in index order.
    Returns S, F, hoods (ncases, K) int32, point_index (ncases,) int32."""
    m = {1: 512, 2: 32, 3: 16}[dim]
    offs, r2 = lattice_shells(dim, K)
    offs = np.concatenate([np.zeros((1, dim), np.int64), offs])[:K]
    reach = int(np.abs(offs).max())
    ax = np.arange(m)
    nodes = np.stack(np.meshgrid(*([ax] * dim), indexing="ij"), axis=-1).reshape(-1, dim)
    S = nodes * GRID_H
    F = f(S)
    inner = np.all((nodes >= reach) & (nodes < m - reach), axis=1)
    centre = nodes[inner]
    nb = centre[:, None, :] + offs[None, :, :]
    strides = m ** np.arange(dim - 1, -1, -1)
    hoods = (nb * strides).sum(axis=-1).astype(np.int32)
    pidx = (centre * strides).sum(axis=-1).astype(np.int32)
    if dim == 1:
        S = np.ascontiguousarray(S[:, 0])
    return S, F, hoods, pidx


# ---- the batches the tests run: four blocks of knowns / weighting per family ---------------------------------------------------------

def combos(n):
    """Per-case knowns and weighting in four equal blocks (whole waves of one kind for n = 256): centre weighting without knowns, centre
    weighting with the function value known (b?_F, the default mask of the reference), uniform weighting without knowns, uniform / F."""
    q = np.arange(n) * 4 // n
    return np.where(q % 2 == 1, 1, 0).astype(np.int64), np.where(q < 2, 2, 1).astype(np.int32)


def truth_job(job):
    """(family, dim, order, K, n, lo, hi) -> (fi, kappa) of cases lo..hi of that batch by `_parity.truth_fit_mp`.  A plain function of
    plain arguments: it runs in worker processes that import numpy and mpmath only."""
    import _parity as P
    family, dim, order, K, n, lo, hi = job
    b = lattice_batch(dim, order, K, n) if family == "lattice" else make(family, dim, order, K, n)
    kn, wm = combos(n)
    s = slice(lo, hi)
    return P.truth_fit_mp(dim, b["xk"][s], b["fk"][s], b["nk"][s], b["xi"][s], b["fi0"][s], b["order_a"][s], kn[s], wm[s])


def _map(fn, jobs, workers):
    if workers <= 1:
        return [fn(j) for j in jobs]
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    with ProcessPoolExecutor(max_workers=workers, mp_context=mp.get_context("spawn")) as ex:
        return list(ex.map(fn, jobs))


def truths(jobs, workers=1):
    """[truth_job(j) for j in jobs], over `workers` freshly started processes when workers > 1."""
    return _map(truth_job, jobs, workers)


# ---- the fit's linear operator: sensitivities and adjoints -----------------------------------------------------------------------------

# The families whose GEOMETRY differs (the operator does not see the data: fk* and exactpoly* share `plain`'s geometry), plus the real
# lattice with self-including rows.  EDGE_EXP and COLLINEAR_EPS apply unchanged (tests/test_adversarial_cpu.py rehearses that the oracle's
# sensitivities and the adjoint built from them stay finite and a reference on every one of them).
OP_FAMILIES = ("plain", "grid", "grid_sorted", "sortedguess", "far", "aniso", "onesided", "self", "collinear", "tiny", "huge", "tiny_edge",
               "huge_edge", "lattice")
# One full wave and one half-filled one; combos(96) puts its four blocks of 24 across them, so that a wave holds several knowns /
# weighting kinds (the fit suite's blocks are whole waves of one kind: this is the complementary arrangement).
N_OP = 96
OP_FIELDS = (0, 2)            # the seeds of g that have a truth; field 1 of a stack is field 0 times -1/2 (exact, truth included)


def op_batch(family, dim, order, K, n=N_OP):
    """The batch of `family` with its knowns / weighting (combos(n)) under the keys kn, wm."""
    b = lattice_batch(dim, order, K, n) if family == "lattice" else make(family, dim, order, K, n)
    b["kn"], b["wm"] = combos(n)
    return b


def op_g(family, dim, order, K, n=N_OP, field=0):
    """g = dL/dfi_out of a family and shape: uniform in [-1, 1], seeded by family, shape and field."""
    return _rng("g%d/%s" % (field, family), dim, order, K, n).uniform(-1.0, 1.0, (n, NDOF[dim][order]))


def operator_job(job):
    """(family, dim, order, K, n, lo, hi[, fields]) -> dict(S, J, kappa, live, kind, adjoint={field: (grad_fk, grad_fi, s)}) of cases
    lo..hi by `_parity.truth_operator_mp` and, contracted in mpmath before anything is rounded, `_parity.truth_adjoint_mp` of
    op_g(..., field) for `fields` (default OP_FIELDS; (): the operator alone).  A plain function of plain arguments, as truth_job is."""
    import _parity as P
    family, dim, order, K, n, lo, hi = job[:7]
    fields = tuple(job[7]) if len(job) > 7 else OP_FIELDS
    b = op_batch(family, dim, order, K, n)
    s = slice(lo, hi)
    op = P.truth_operator_mp(dim, b["xk"][s], b["nk"][s], b["xi"][s], b["order_a"][s], b["kn"][s], b["wm"][s], as_mp=True)
    adj = {f: P.truth_adjoint_mp(op, op_g(family, dim, order, K, n, f)[s]) for f in fields}
    return dict(S=op.S.astype(np.float64), J=op.J.astype(np.float64), kappa=op.kappa, live=op.live, kind=op.kind, adjoint=adj)


def operators(jobs, workers=1):
    """[operator_job(j) for j in jobs], over `workers` freshly started processes when workers > 1."""
    return _map(operator_job, jobs, workers)


def operator_truth(family, dim, order, K, n=N_OP, results=None):
    """The pieces of operator_job over consecutive slices of one family joined into one dict (results: the jobs' outputs in order;
    None: computed here in one piece)."""
    results = [operator_job((family, dim, order, K, n, 0, n))] if results is None else results
    out = {k: np.concatenate([r[k] for r in results]) for k in ("S", "J", "kappa", "live", "kind")}
    out["adjoint"] = {f: tuple(np.concatenate([r["adjoint"][f][i] for r in results]) for i in range(3)) for f in results[0]["adjoint"]}
    return out


def lattice_batch(dim, order, K, n):
    """n cases of lattice_cloud (drawn without replacement, seeded) in the dense layout, with the index-based form alongside:
    S, F, hoods, pidx.  Slot 0 of every row is the node itself."""
    S, F, hoods, pidx = lattice_cloud(dim, K)
    rng = _rng("lattice", dim, order, K, n)
    sel = np.sort(rng.choice(len(pidx), n, replace=False))
    hoods, pidx = np.ascontiguousarray(hoods[sel]), np.ascontiguousarray(pidx[sel])
    no = NDOF[dim][order]
    fi0 = rng.uniform(-1, 1, (n, no)); fi0[:, 0] = F[pidx]
    return dict(family="lattice", dim=dim, order=order, K=K, n=n, no=no, xk=np.ascontiguousarray(S[hoods]), fk=np.ascontiguousarray(F[hoods]),
                nk=np.full(n, K, np.int32), xi=np.ascontiguousarray(S[pidx]), fi0=fi0, order_a=np.full(n, order, np.int32),
                S=S, F=F, hoods=hoods, pidx=pidx)
