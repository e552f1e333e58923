"""Reference statements for coupled solves with a per-point coupling (wlsqm.hip.StencilSystemSolver with a device tensor
(m, m, nop, npoints), csrc/krylov.hip), numpy only, on tests/_krylov_system_ref.py.

    M[(i, a), (j, b)] = D_ab,i delta_ij + sum_o c[a, b, o, i] A_o[i, j]          (the equation of point i carries its own coefficients)

The order of operations of the forward product, stated once (product_statement), y = M x for point i:
    for every stored entry e of row i, in entry order, with column k and the values val_o:
        s[o][b] = fma(val_o, x[k, b], s[o][b])                                   for o = 0 .. nop - 1, b = 0 .. m - 1, from s = 0
    t_a = c[a, 0, 0, i] * s[0][0];  t_a = fma(c[a, b, o, i], s[o][b], t_a)       b outer, o inner, (b, o) = (0, 0) left out
    s_a = D_a0,i * x[i, 0];  s_a = fma(D_ab,i, x[i, b], s_a) for b = 1 .. m - 1;  y[i, a] = t_a + s_a
of the transposed product y = M^T lam (mix_statement, transposed_product_statement):
    z[i][o][b] = c[0, b, o, i] * lam[i, 0];  z[i][o][b] = fma(c[a, b, o, i], lam[i, a], z[i][o][b]) for a = 1 .. m - 1
    for every stored entry e of row j of the transposed planes (R.transpose_rows' order), with column i and the values val_o:
        acc_b = fma(val_o, z[i][o][b], acc_b)                                    o outer, b inner, from acc = 0
    s_b = D_0b,j * lam[j, 0];  s_b = fma(D_ab,j, lam[j, a], s_b) for a = 1 .. m - 1;  y[j, b] = acc_b + s_b
and of the Jacobi diagonal (jacobi_statement), own_o the sum of row i's entries of plane o in column i in entry order:
    t = c[a, a, 0, i] * own_0;  t = t + c[a, a, o, i] * own_o for o = 1 .. nop - 1;  diagonal = D_aa,i + t
The gradient kernel is tests/_krylov_system_adjoint_ref.grads_statement with c[:, :, :, j] for row j (grads_statement).

Rounding: a term c val x of the forward product passes through the len roundings of its s chain, at most m nop of the contraction and
the last sum: T = len + m nop + 1 (forward_chain).  Transposed: m of the mix, nop len of the acc chain and the last sum:
T = m + nop len + 1 (transposed_chain).  The terms of the diag part pass through m + 1, which is never more.

The systems whose iteration counts stand behind the GPU tests' caps (SYSTEMS, system): the three elasticity clouds of
_krylov_system_ref with f = sin(2 pi x) cos(2 pi y), mu = 1 + 0.5 f, lambda = 1 - 0.5 f in elasticity_coupling's formula per point, and
the scalar diffusion step I - 0.25 h^2 (k Lap + k_x d/dx + k_y d/dy), k = 1 + 0.5 f, on the cloud of 2D-tau0.25-n130.  CAPS[name][pc] and
TRANSPOSED_CAPS[name][pc] are twice the count of _krylov_ref.bicgstab_ref (zero start, rtol 1e-10; the system's own b, and
_krylov_system_adjoint_ref.adjoint_rhs for M^T) on the oracle's coefficients, which tests/test_krylov_system_point_host.py holds the
constants to.  HOST_ONLY: the (name, preconditioner, transposed) whose count the reversed summation order moves by 1.25x or more."""
from fractions import Fraction

import numpy as np

import _krylov_ref as KR
import _krylov_system_adjoint_ref as SA
import _krylov_system_ref as SR
import _stencil_ref as R

fma = SR.fma
CONTRAST = 0.5

SYSTEMS = ("elasticity-2D-n130", "elasticity-2D-n1000", "elasticity-3D-n1000", "diffusion-2D-n130")

# name: {preconditioner: maxiter}, twice the reference's count (tests/test_krylov_system_point_host.py)
CAPS = {
    "elasticity-2D-n130": {"jacobi": 82, None: 72},
    "elasticity-2D-n1000": {"jacobi": 526, None: 262},
    "elasticity-3D-n1000": {"jacobi": 86, None: 106},
    "diffusion-2D-n130": {"jacobi": 20, None: 16},
}
TRANSPOSED_CAPS = {
    "elasticity-2D-n130": {"jacobi": 80, None: 74},
    "elasticity-2D-n1000": {"jacobi": 392, None: 258},
    "elasticity-3D-n1000": {"jacobi": 74, None: 128},
    "diffusion-2D-n130": {"jacobi": 18, None: 16},
}
HOST_ONLY = []
CASES = [(name, pc, tr) for tr, caps in ((False, CAPS), (True, TRANSPOSED_CAPS)) for name in SYSTEMS for pc in caps[name]]
GPU_CASES = [c for c in CASES if c not in HOST_ONLY]


def constant_table(coupling, n):
    """(m, m, nop, n): a table (m, m, nop) repeated at every point."""
    coupling = np.asarray(coupling, np.float64)
    return np.ascontiguousarray(np.broadcast_to(coupling[..., None], coupling.shape + (n,)))


def dense_matrix(A, cpt, diag):
    """The dense M (m n, m n) of the interleaved numbering: block (a, b) is D_ab + sum_o diag(c[a, b, o, :]) A_o."""
    cpt = np.asarray(cpt, np.float64)
    m, n = cpt.shape[0], A.shape[1]
    M = np.einsum("aboi,oij->iajb", cpt, A)
    D = SR.diag_blocks(diag, m, n)
    i = np.arange(n)
    M[i, :, i, :] += np.transpose(D, (2, 0, 1))
    return np.ascontiguousarray(M.reshape(m * n, m * n))


def forward_chain(lens, m, nop):
    """The longest chain of roundings a term of the forward product passes through, per row."""
    return np.asarray(lens) + m * nop + 1


def transposed_chain(tlens, m, nop):
    """The same for the transposed product, per row of the transposed planes."""
    return m + nop * np.asarray(tlens) + 1


def product_statement(rows, cpt, diag, x):
    """y (n, m) = M x in the stated order of operations, every fma rounded once: what krylov-system-spmv-point's bits are."""
    cpt = np.asarray(cpt, np.float64)
    m, nop, n = cpt.shape[0], cpt.shape[2], len(rows)
    D = SR.diag_blocks(diag, m, n)
    y = np.zeros((n, m))
    for i, row in enumerate(rows):
        s = [[0.0] * m for _ in range(nop)]
        for k, v in row:
            for o in range(nop):
                for b in range(m):
                    s[o][b] = fma(v[o], x[k, b], s[o][b])
        for a in range(m):
            t = cpt[a, 0, 0, i] * s[0][0]
            for b in range(m):
                for o in range(nop):
                    if b + o > 0:
                        t = fma(cpt[a, b, o, i], s[o][b], t)
            sa = D[a, 0, i] * x[i, 0]
            for b in range(1, m):
                sa = fma(D[a, b, i], x[i, b], sa)
            y[i, a] = t + sa
    return y


def mix_statement(cpt, lam):
    """z (n, nop, m): krylov-system-mix's bits."""
    cpt = np.asarray(cpt, np.float64)
    m, nop, n = cpt.shape[0], cpt.shape[2], cpt.shape[3]
    z = np.zeros((n, nop, m))
    for i in range(n):
        for o in range(nop):
            for b in range(m):
                t = cpt[0, b, o, i] * lam[i, 0]
                for a in range(1, m):
                    t = fma(cpt[a, b, o, i], lam[i, a], t)
                z[i, o, b] = t
    return z


def transposed_product_statement(rows, cpt, diag, lam):
    """y (n, m) = M^T lam in the stated order of operations: krylov-system-mix, then krylov-system-spmv-mixed on the transposed rows."""
    cpt = np.asarray(cpt, np.float64)
    m, nop, n = cpt.shape[0], cpt.shape[2], len(rows)
    D = SR.diag_blocks(diag, m, n)
    z = mix_statement(cpt, lam)
    y = np.zeros((n, m))
    for j, row in enumerate(R.transpose_rows(rows, n)):
        acc = [0.0] * m
        for i, v in row:
            for o in range(nop):
                for b in range(m):
                    acc[b] = fma(v[o], z[i, o, b], acc[b])
        for b in range(m):
            s = D[0, b, j] * lam[j, 0]
            for a in range(1, m):
                s = fma(D[a, b, j], lam[j, a], s)
            y[j, b] = acc[b] + s
    return y


def exact_sum_of_products(f1, f2, f3):
    """(sum f1_i f2_i f3_i, sum |f1_i f2_i f3_i|) of finite float arrays as Fractions, in integer arithmetic (_krylov_ref.exact_dot's
    method with three factors: a transposed row may hold tens of thousands of entries)."""
    ints, exps = [], 0
    for f in (f1, f2, f3):
        mant, e = np.frexp(np.ravel(np.asarray(f, np.float64)))
        ints.append(np.ldexp(mant, 53).astype(np.int64).tolist())
        exps = exps + e.astype(np.int64) - 53
    exps = exps.tolist() if len(ints[0]) else []
    emin = min(exps) if exps else 0
    total = mag = 0
    for a, b, c, k in zip(ints[0], ints[1], ints[2], exps):
        term = (a * b * c) << (k - emin)
        total += term
        mag += abs(term)
    two = Fraction(2) ** emin
    return total * two, mag * two


def exact_product(rows, cpt, diag, x, check=None, transposed=False, trows=None):
    """(exact, mag) (len(check), m): per unknown the exact value of (M x), or of (M^T x), rounded once, and the sum of the magnitudes of
    its terms c * val * x and D * x: the dense statement in exact arithmetic on the rows `check` (default: all).  trows: the
    transposed rows, when the caller has them."""
    cpt = np.asarray(cpt, np.float64)
    m, nop, n = cpt.shape[0], cpt.shape[2], len(rows)
    D = SR.diag_blocks(diag, m, n)
    check = range(n) if check is None else check
    trows = (R.transpose_rows(rows, n) if trows is None else trows) if transposed else None
    exact, mag = np.zeros((len(check), m)), np.zeros((len(check), m))
    for k, i in enumerate(check):
        row = trows[i] if transposed else rows[i]
        cols = np.array([c for c, _ in row], np.int64)
        V = np.array([v for _, v in row], np.float64).reshape(len(row), nop)[:, None, :]          # (len, 1, nop)
        X = x[cols][:, :, None]                                                                     # (len, m, 1)
        shape = (len(row), m, nop)
        for a in range(m):
            if transposed:                                      # unknown (i, a) of M^T x: the rows j that name column i, c[c', a, o, j]
                C, Dx = np.transpose(cpt[:, a, :, :][:, :, cols], (2, 0, 1)), D[:, a, i]
            else:                                               # unknown (i, a) of M x: c[a, b, o, i]
                C, Dx = cpt[a, :, :, i][None], D[a, :, i]
            f = [np.broadcast_to(t, shape).ravel() for t in (C, V, X)]
            total, size = exact_sum_of_products(np.r_[f[0], Dx], np.r_[f[1], x[i]], np.r_[f[2], np.ones(m)])
            exact[k, a], mag[k, a] = float(total), float(size)
    return exact, mag


def jacobi_statement(rows, cpt, diag):
    """(m n,): the scalar diagonal of M as krylov-system-diag-point forms it (its inverse is the preconditioner)."""
    cpt = np.asarray(cpt, np.float64)
    m, nop, n = cpt.shape[0], cpt.shape[2], len(rows)
    D = SR.diag_blocks(diag, m, n)
    out = np.zeros((n, m))
    for i, row in enumerate(rows):
        own = np.zeros(nop)
        for c, v in row:
            if c == i:
                own = own + v
        for a in range(m):
            t = cpt[a, a, 0, i] * own[0]
            for o in range(1, nop):
                t = t + cpt[a, a, o, i] * own[o]
            out[i, a] = D[a, a, i] + t
    return out.reshape(-1)


def grads_statement(sell, n, cpt, lam, x, check=None):
    """_krylov_system_adjoint_ref.grads_statement with row j's own coefficients c[:, :, :, j]: (at, values (nop, len(at)), diag)."""
    cpt = np.asarray(cpt, np.float64)
    m, nop = cpt.shape[0], cpt.shape[2]
    check = np.arange(n) if check is None else np.asarray(check)
    at, vals, diag = [], [], np.zeros((m, m, len(check)))
    for k, j in enumerate(check):
        a_j, v_j, d_j = SA.grads_statement(sell, n, cpt[:, :, :, j], lam, x, [j])
        at.append(a_j); vals.append(v_j)
        diag[:, :, k] = d_j[:, :, 0]
    return (np.concatenate(at) if at else np.zeros(0, np.int64)), (np.concatenate(vals, axis=1) if vals else np.zeros((nop, 0))), diag


def coupling_gradient_statement(A, lam, x):
    """(exact-order-free value, mag) (m, m, nop, n) of dL/dc[a, b, o, i] = -lam[i, a] (A_o x[:, b])_i and the magnitude
    |lam[i, a]| (|A_o| |x[:, b]|)_i that the rounding of the product A_o x and of the one multiplication is measured in."""
    Y = np.einsum("oij,jb->boi", A, x)
    Ymag = np.einsum("oij,jb->boi", np.abs(A), np.abs(x))
    return -(lam.T[:, None, None, :] * Y[None]), np.abs(lam.T)[:, None, None, :] * Ymag[None]


def implicit_gradients(A, cpt, diag, b, g):
    """_krylov_system_adjoint_ref.implicit_gradients for a per-point table: coupling (m, m, nop, n) = -lam[i, a] (A_o x[:, b])_i and
    entries (nop, n, n) = -sum_ab c[a, b, o, j] lam[j, a] x[k, b], by dense solves."""
    cpt = np.asarray(cpt, np.float64)
    n, m = b.shape
    M = dense_matrix(A, cpt, diag)
    x = np.linalg.solve(M, b.reshape(-1)).reshape(n, m)
    lam = np.linalg.solve(M.T, g.reshape(-1)).reshape(n, m)
    return dict(x=x, lam=lam, b=lam, diag=-np.einsum("ia,ib->abi", lam, x), coupling=-np.einsum("ia,oij,jb->aboi", lam, A, x),
                entries=-np.einsum("aboj,ja,kb->ojk", cpt, lam, x), M=M)


def geometry_truth(sy, cpt, x, lam):
    """_krylov_system_adjoint_ref.geometry_truth with g_j = -sum_o (sum_a c[a, b, o, j] lam[j, a]) rows[o]."""
    import _geometry_adjoint_ref as GA
    n, dim, S, hoods, m = sy["n"], sy["dim"], sy["S"], sy["hoods"], sy["m"]
    rows = sy["rows"]
    no = rows.shape[-1]
    per_case = np.broadcast_to(rows if rows.ndim == 3 else rows[:, None, :], (rows.shape[0], n, no))
    T = np.zeros_like(S)
    for b in range(m):
        u = np.einsum("aoj,ja->jo", cpt[:, b], lam)
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


def field(S):
    """f = sin(2 pi x) cos(2 pi y) at the points, and its derivatives to x and y."""
    X, Y = 2.0 * np.pi * S[:, 0], 2.0 * np.pi * S[:, 1]
    return np.sin(X) * np.cos(Y), 2.0 * np.pi * np.cos(X) * np.cos(Y), -2.0 * np.pi * np.sin(X) * np.sin(Y)


def elasticity_table(dim, mu, lam):
    """(dim, dim, nop, n): _krylov_system_ref.elasticity_coupling's formula with the Lame parameters of every point."""
    one = SR.elasticity_coupling(dim)                                   # at lambda = mu = 1: which entries carry what
    pure = {2: [0, 2], 3: [0, 2, 4]}[dim]
    nop, n = one.shape[2], len(mu)
    cp = np.zeros((dim, dim, nop, n))
    for a in range(dim):
        for p in pure:
            cp[a, a, p] -= mu
        cp[a, a, pure[a]] -= lam + mu
        cp[a, a, nop - 1] = 1.0
        for b in range(dim):
            if a != b:
                cp[a, b, int(np.flatnonzero(one[a, b])[0])] = -(lam + mu)
    return cp


_systems = {}


def system(name):
    """_krylov_system_ref.system's dict with `coupling` the per-point table (m, m, nop, n); computed once."""
    if name in _systems:
        return _systems[name]
    if name.startswith("elasticity"):
        sy = dict(SR.system(name))
        f = field(sy["S"])[0]
        sy["coupling"] = elasticity_table(sy["dim"], 1.0 + CONTRAST * f, 1.0 - CONTRAST * f)
    else:
        import wlsqm
        sb = KR.system("2D-tau0.25-n130")
        n, dim = sb["n"], sb["dim"]
        h = n ** (-1.0 / dim)
        rows = np.zeros((3, len(KR.laplacian_row(dim))))
        rows[0] = KR.laplacian_row(dim)
        rows[1, wlsqm.i2_X] = 1.0
        rows[2, wlsqm.i2_Y] = 1.0
        f, fx, fy = field(sb["S"])
        cpt = np.zeros((1, 1, 3, n))
        cpt[0, 0] = -0.25 * h * h * np.stack([1.0 + CONTRAST * f, CONTRAST * fx, CONTRAST * fy])
        b = np.random.default_rng([61, n, 1]).standard_normal((n, 1))
        sy = dict(kind="diffusion", m=1, nop=3, n=n, dim=dim, order=2, S=sb["S"], hoods=sb["hoods"], nk=sb["nk"], knowns=sb["knowns"],
                  wm=sb["wm"], rows=rows, band=sb["band"], coupling=cpt, diag=1.0, b=b)
    _systems[name] = sy
    return sy


def dense_of(sy, A=None):
    """The dense M of a per-point system; A: the dense planes (the GPU tests pass the library's own), default the oracle's."""
    return dense_matrix(SR.oracle_planes(sy) if A is None else A, sy["coupling"], sy["diag"])
