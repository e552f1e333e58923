"""Reference statements for the coupled solves (wlsqm.hip.StencilSystemSolver, csrc/krylov.hip), numpy only.

m unknowns per point, interleaved: unknown (i, a), component a at point i, has the number i m + a.  Block (a, b) of M is
D_ab + sum_o coupling[a, b, o] A_o, A_o the value planes of one square structure, D_ab a diagonal matrix (`diag`: a float d for d I_m,
an (m, m) array of constants, or an (m, m, n) array).

The order of operations of the product, stated once (product_statement), y = M x for point i:
    for every stored entry e of row i, in entry order, with column c and the values val_o:
        for a = 0 .. m - 1, for b = 0 .. m - 1:
            t = coupling[a, b, 0] * val_0;  t = fma(coupling[a, b, o], val_o, t) for o = 1 .. nop - 1
            acc_a = fma(t, x[c, b], acc_a)
    s_a = D_a0,i * x[i, 0];  s_a = fma(D_ab,i, x[i, b], s_a) for b = 1 .. m - 1
    y[i, a] = acc_a + s_a
and of the Jacobi diagonal (jacobi_statement), for unknown (i, a), own_o the sum of row i's entries of plane o in column i in entry order:
    t = coupling[a, a, 0] * own_0;  t = t + coupling[a, a, o] * own_o for o = 1 .. nop - 1;  diagonal = D_aa,i + t
A lane's terms of a dot product are added for a = 0 .. m - 1, then the lanes go through the fixed tree of the single-field kernels.

The systems (SYSTEMS): the three elasticity systems of the rehearsal on clouds in Morton order (_krylov_block_ref.morton_system), a
reaction-diffusion pair, and random structures for every m.  CAPS[name] is the `maxiter` of the GPU tests: twice the count of
_krylov_ref.bicgstab_ref (Jacobi, zero start, rtol 1e-10) on the oracle's coefficients, which tests/test_krylov_system_host.py holds the
constant to.  HOST_ONLY: the systems whose count moves by 1.25x or more under the reversed summation order."""
from fractions import Fraction

import numpy as np

import _krylov_ref as KR
import _stencil_ref as R

EPS = 2.0 ** -53
LAMBDA = MU = 1.0

# name: (kind, base system of _krylov_ref whose cloud it takes, m)
SYSTEMS = {
    "elasticity-2D-n130": ("elasticity", "2D-dirichlet-n130", 2),
    "elasticity-2D-n1000": ("elasticity", "2D-dirichlet-n1000", 2),
    "elasticity-3D-n1000": ("elasticity", "3D-dirichlet-n1000", 3),
    "reaction-2D-n130": ("reaction", "2D-tau0.25-n130", 2),
    "random-m1": ("random", None, 1),
    "random-m2": ("random", None, 2),
    "random-m3": ("random", None, 3),
    "random-m4": ("random", None, 4),
}
RANDOM_NOP = {1: 1, 2: 3, 3: 4, 4: 7}
RANDOM_N, RANDOM_K = 300, 9

# name: {"jacobi": maxiter, None: maxiter}, twice the reference's count (tests/test_krylov_system_host.py)
CAPS = {
    "elasticity-2D-n130": {"jacobi": 80, None: 82},
    "elasticity-2D-n1000": {"jacobi": 426, None: 262},
    "elasticity-3D-n1000": {"jacobi": 80, None: 86},
    "reaction-2D-n130": {"jacobi": 20, None: 18},
    "random-m1": {"jacobi": 14, None: 32},
    "random-m2": {"jacobi": 26, None: 110},
    "random-m3": {"jacobi": 26, None: 146},
    "random-m4": {"jacobi": 30, None: 190},
}

# (name, preconditioner) whose count the reversed summation order moves by 1.25x or more: no yardstick for a device whose sums run in
# yet another order.  tests/test_krylov_system_host.py holds the list to the rule.
HOST_ONLY = []
GPU_CASES = [(name, pc) for name, caps in CAPS.items() for pc in caps if (name, pc) not in HOST_ONLY]


def fma(a, b, c):
    """a * b + c rounded once."""
    a, b, c = float(a), float(b), float(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def diag_blocks(diag, m, n):
    """(m, m, n): the three forms of `diag` as one array."""
    d = np.asarray(diag, np.float64)
    if d.ndim == 0:
        return float(d) * np.broadcast_to(np.eye(m)[:, :, None], (m, m, n)).copy()
    if d.ndim == 2:
        return np.broadcast_to(d[:, :, None], (m, m, n)).copy()
    return d


def planes_structure(nrows, K, nop, seed):
    """_krylov_ref.square_structure with nop value planes: the same hoods, nk and own_mask, the planes drawn afresh (NaN in the padding)."""
    st = KR.square_structure(nrows, K, seed)
    rng = np.random.default_rng([seed, nrows, K, nop, 5])
    slots = rng.standard_normal((nop, nrows, K))
    own = rng.standard_normal((nop, nrows))
    slots[:, np.isnan(st["slots"][0])] = np.nan
    own[:, np.isnan(st["own"][0])] = np.nan
    return dict(st, slots=slots, own=own)


def rows_of_structure(st):
    return R.rows_of(st["hoods"], st["nk"], st["slots"], st["own"], st["own_mask"], st["pts"])


def dense_planes(rows, n, nop):
    """(nop, n, n): every plane dense, the duplicates of a row summed in entry order."""
    return np.stack([R.dense(rows, n, o) for o in range(nop)])


def dense_matrix(A, coupling, diag):
    """The dense M (m n, m n) of the interleaved numbering from the dense planes A (nop, n, n), coupling (m, m, nop) and diag."""
    coupling = np.asarray(coupling, np.float64)
    m, n = coupling.shape[0], A.shape[1]
    M = np.einsum("abo,oij->iajb", coupling, A)
    D = diag_blocks(diag, m, n)
    i = np.arange(n)
    M[i, :, i, :] += np.transpose(D, (2, 0, 1))
    return np.ascontiguousarray(M.reshape(m * n, m * n))


def product_statement(rows, coupling, diag, x):
    """y (n, m) = M x in the stated order of operations, every fma rounded once: what the kernel's bits are."""
    coupling = np.asarray(coupling, np.float64)
    m, nop, n = coupling.shape[0], coupling.shape[2], len(rows)
    D = diag_blocks(diag, m, n)
    y = np.zeros((n, m))
    for i, row in enumerate(rows):
        acc = [0.0] * m
        for c, v in row:
            for a in range(m):
                for b in range(m):
                    t = coupling[a, b, 0] * v[0]
                    for o in range(1, nop):
                        t = fma(coupling[a, b, o], v[o], t)
                    acc[a] = fma(t, x[c, b], acc[a])
        for a in range(m):
            s = D[a, 0, i] * x[i, 0]
            for b in range(1, m):
                s = fma(D[a, b, i], x[i, b], s)
            y[i, a] = acc[a] + s
    return y


def exact_product(rows, coupling, diag, x, check=None):
    """(exact, mag) (len(check), m): per unknown the exact value of (M x) rounded once, and the sum of the magnitudes of its terms
    coupling * val * x and D * x: the dense statement in exact arithmetic on the rows `check` (default: all)."""
    coupling = np.asarray(coupling, np.float64)
    m, nop, n = coupling.shape[0], coupling.shape[2], len(rows)
    D = diag_blocks(diag, m, n)
    check = range(n) if check is None else check
    exact, mag = np.zeros((len(check), m)), np.zeros((len(check), m))
    F = lambda v: Fraction(float(v))
    for k, i in enumerate(check):
        for a in range(m):
            terms = [F(coupling[a, b, o]) * F(v[o]) * F(x[c, b]) for c, v in rows[i] for b in range(m) for o in range(nop)]
            terms += [F(D[a, b, i]) * F(x[i, b]) for b in range(m)]
            exact[k, a] = float(sum(terms, Fraction(0)))
            mag[k, a] = float(sum((abs(t) for t in terms), Fraction(0)))
    return exact, mag


def jacobi_statement(rows, coupling, diag):
    """(m n,): the scalar diagonal of M as the diagonal kernel forms it (its inverse is the preconditioner)."""
    coupling = np.asarray(coupling, np.float64)
    m, nop, n = coupling.shape[0], coupling.shape[2], len(rows)
    D = diag_blocks(diag, m, n)
    out = np.zeros((n, m))
    for i, row in enumerate(rows):
        own = np.zeros(nop)
        for c, v in row:
            if c == i:
                own = own + v
        for a in range(m):
            t = coupling[a, a, 0] * own[0]
            for o in range(1, nop):
                t = t + coupling[a, a, o] * own[o]
            out[i, a] = D[a, a, i] + t
    return out.reshape(-1)


def elasticity_coupling(dim):
    """(dim, dim, nop): -(mu Lap u + (lambda + mu) grad div u) on the second-derivative planes, and 1 on the last plane (`value`: the
    identity rows of the boundary band) in every diagonal block.  Planes: X2, XY, Y2, value in 2D; X2, XY, Y2, YZ, Z2, XZ, value in 3D."""
    pure = {2: [0, 2], 3: [0, 2, 4]}[dim]                              # d2/dx_a^2
    mixed = {2: {(0, 1): 1}, 3: {(0, 1): 1, (1, 2): 3, (0, 2): 5}}[dim]
    nop = {2: 4, 3: 7}[dim]
    cp = np.zeros((dim, dim, nop))
    for a in range(dim):
        for p in pure:
            cp[a, a, p] -= MU
        cp[a, a, pure[a]] -= LAMBDA + MU
        cp[a, a, nop - 1] = 1.0
        for b in range(dim):
            if a != b:
                cp[a, b, mixed[min(a, b), max(a, b)]] = -(LAMBDA + MU)
    return cp


def second_derivative_rows(dim):
    """(nop - 1, no): the rows of the second derivatives over the order-2 DOFs, in the order of elasticity_coupling's planes."""
    import wlsqm
    names = {2: ("X2", "XY", "Y2"), 3: ("X2", "XY", "Y2", "YZ", "Z2", "XZ")}[dim]
    no = {2: 6, 3: 10}[dim]
    rows = np.zeros((len(names), no))
    for o, name in enumerate(names):
        rows[o, getattr(wlsqm, "i%d_%s" % (dim, name))] = 1.0
    return rows


_systems = {}


def system(name):
    """What a test needs to build the system `name` on either side: dict(kind, m, nop, n, coupling, diag, b (n, m)) and, for a fit,
    dim, order, S, hoods, nk, knowns, wm, rows (nop, n, no) or (nop, no), band; for a random structure, st.  Computed once."""
    if name in _systems:
        return _systems[name]
    kind, base, m = SYSTEMS[name]
    if kind == "random":
        nop, n = RANDOM_NOP[m], RANDOM_N
        st = planes_structure(n, RANDOM_K, nop, seed=53 + m)
        rng = np.random.default_rng([59, m])
        coupling = rng.standard_normal((m, m, nop))
        A = dense_planes(rows_of_structure(st), n, nop)
        off = rng.standard_normal((m, m, n))
        for a in range(m):
            off[a, a] = 0.0
        M0 = dense_matrix(A, coupling, off)
        dom = 1.0 + 1.5 * np.abs(M0).sum(axis=1).reshape(n, m)
        diag = off.copy()
        for a in range(m):
            diag[a, a] = dom[:, a]
        sy = dict(kind=kind, m=m, nop=nop, n=n, st=st, coupling=coupling, diag=diag, b=rng.standard_normal((n, m)))
    else:
        import _krylov_block_ref as KB
        sb = KB.morton_system(base) if kind == "elasticity" else KR.system(base)
        dim, n = sb["dim"], sb["n"]
        rng = np.random.default_rng([61, n, m])
        b = rng.standard_normal((n, m))
        if kind == "elasticity":
            d2 = second_derivative_rows(dim)
            no = d2.shape[1]
            band = sb["band"]
            rows = np.zeros((d2.shape[0] + 1, n, no))
            rows[:-1] = np.where(band[None, :, None], 0.0, d2[:, None, :])
            rows[-1, band, 0] = 1.0
            coupling, diag = elasticity_coupling(dim), 0.0
        else:
            h = n ** (-1.0 / dim)
            rows = KR.laplacian_row(dim)[None, :].copy()
            coupling = np.zeros((m, m, 1))
            coupling[0, 0, 0] = coupling[1, 1, 0] = -0.25 * h * h
            diag = np.eye(m) + np.array([[0.5, -0.3], [0.2, 0.4]])
        sy = dict(kind=kind, m=m, nop=coupling.shape[2], n=n, dim=dim, order=2, S=sb["S"], hoods=sb["hoods"], nk=sb["nk"],
                  knowns=sb["knowns"], wm=sb["wm"], rows=rows, band=sb["band"], coupling=coupling, diag=diag, b=b)
    _systems[name] = sy
    return sy


def oracle_planes(sy):
    """(nop, n, n): the dense planes of a system from the CPU oracle's coefficients (a fit), or from the structure itself."""
    n, nop = sy["n"], sy["nop"]
    if sy["kind"] == "random":
        return dense_planes(rows_of_structure(sy["st"]), n, nop)
    import _adjoint_ref as AD
    out = []
    for o in range(nop):
        g = np.ascontiguousarray(np.broadcast_to(sy["rows"][o], (n, sy["rows"].shape[-1])))
        ref = AD.adjoint_ref(sy["dim"], sy["order"], np.ascontiguousarray(sy["S"][sy["hoods"]]), sy["nk"], sy["S"], sy["knowns"], sy["wm"], g)
        rows = R.rows_of(sy["hoods"], sy["nk"], ref["grad_fk"][None], ref["grad_fi"][None, :, 0], np.ones(n, bool), np.arange(n))
        out.append(R.dense(rows, n, 0))
    return np.stack(out)


def dense_of(sy, A=None):
    """The dense M of a system; A: the dense planes (the GPU tests pass the library's own), default oracle_planes."""
    return dense_matrix(oracle_planes(sy) if A is None else A, sy["coupling"], sy["diag"])


def solve_ref(M, b, precond, cap=20000, reverse=False, x0=None):
    """_krylov_ref.bicgstab_ref at rtol 1e-10; reverse: on the system with rows and columns reversed (another summation order), x
    returned in the matrix's own order.  b and x are flat (m n,)."""
    n = len(b)
    x0 = np.zeros(n) if x0 is None else x0
    if reverse:
        Mr = np.ascontiguousarray(M[::-1, ::-1])
        x, its, status, hist = KR.bicgstab_ref(Mr, b[::-1].copy(), x0[::-1].copy(), KR.jacobi(Mr) if precond == "jacobi" else None, KR.RTOL, 0.0, cap)
        return x[::-1], its, status, hist
    return KR.bicgstab_ref(M, b, x0, KR.jacobi(M) if precond == "jacobi" else None, KR.RTOL, 0.0, cap)
