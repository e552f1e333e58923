"""Truth and reference of the fit's GEOMETRY adjoint (wlsqm.hip.fit_many_geometry_adjoint_device): the gradient of
L = g . fi_out with respect to the coordinates xk and xi of a fit.

With d_k = xk_k - xi, c_k the scaled monomials of d_k, U / Kn / D the unknown, truly known and dropped DOFs, phi = fi_out with the entries
in D replaced by 0, y_U = M_UU^-1 g_U (y = 0 outside U), s_k = c_k . y, r_k = fk_k - c_k . phi and (d_m c)[a] the scaled monomial whose
exponent on axis m is one lower (0 when that exponent is 0), for k < nk

    e[k][m] = (dw_k/dd_k,m) s_k r_k + w_k (r_k (d_m c_k . y) - s_k (d_m c_k . phi)),

dw = 0 under uniform weights; otherwise, with beta = 1 - 1e-4, D2 = max_k d2_k, rho_k = sqrt(d2_k / D2), t_k = 1 - rho_k,

    dw_k/dd_k,m = -2 beta t_k d_k,m / (rho_k D2)          (0 where rho_k == 0: the cone of |d| at d = 0 contributes nothing),
    E           = sum_k (beta t_k rho_k / D2) s_k r_k,
    e[k*][m]   += 2 d_k*,m E                              (k* the SMALLEST index that attains D2: a tie goes to the smaller index),

and grad_xk[k][m] = e[k][m] (exact zeros for nk <= k < K), grad_xi[m] = -sum_k e[k][m], grad_fk[k] = w_k s_k.  A case with every DOF known
has zeros everywhere.

Three statements of it, which share the formula and nothing else:
  truth_geometry_adjoint_mp   mpmath on `_parity._system_mp` and `_parity.truth_fit_mp(as_mp=True)`, rounded once at the end; k* from exact
                              arithmetic.  tests/test_geometry_adjoint_cpu.py pins it to central differences of `fit_value_mp`.
  fit_value_mp                g . fi_out as a function of mpmath coordinates (a double cannot hold a step of 1e-25 of the neighbourhood):
                              the fit restated on plain normal equations, for the difference quotients only.
  geometry_adjoint_ref        fp64 numpy: column-equilibrated normal equations, a LAPACK solve, phi from the CPU oracle's fit.  It does not
                              touch the kernels; the GPU result is judged against it.
The scale s[j] of a case is the largest, over (k, m), of the sum of the absolute values of the terms of e[k][m], or 1 where that is 0.  A
term is one product of the formula as an fp64 evaluation adds them up: (dw) s r; w r (d_m c)[a] y[a] and w s (d_m c)[a] phi[a] for every
DOF a; for slot k*, 2 d_k*,m (beta t_k rho_k / D2) s_k r_k for every k.  r_k and s_k are factors, not expanded: the cancellation inside
them is not counted into the scale."""
import numpy as np

import _adversarial as A
import _parity as P

ALPHA = 1e-4


def lowered(dim, order):
    """low[m][a]: the index of the DOF whose exponent on axis m is one lower than DOF a's, -1 where that exponent is 0."""
    ex = [tuple(e) for e in P.exponents(dim, order)]
    where = {e: a for a, e in enumerate(ex)}
    low = []
    for m in range(dim):
        row = []
        for e in ex:
            if e[m] == 0:
                row.append(-1)
            else:
                t = list(e); t[m] -= 1
                row.append(where[tuple(t)])
        low.append(row)
    return low


def _order_array(order, n):
    return np.full(n, order, np.int32) if np.isscalar(order) else np.asarray(order, np.int32)


def truth_geometry_adjoint_mp(dim, xk, fk, nk, xi, fi_in, order, knowns, wm, g, dps=60, as_mp=False):
    """(grad_xk (n, K, dim), grad_xi (n, dim), s (n,), kappa (n,)) in float64, from mpmath at `dps` digits and rounded once at the end
    (as_mp=True: the two gradients as object arrays of mpf, before that rounding).  1D: xk (n, K), xi (n,); the outputs keep the trailing
    axis of length 1.  order: an int or a per-case array."""
    from mpmath import mp, mpf
    n = len(nk)
    order = _order_array(order, n)
    K = int(np.asarray(xk).shape[1])
    kind = object if as_mp else np.float64
    gxk, gxi, s_out = np.zeros((n, K, dim), kind), np.zeros((n, dim), kind), np.ones(n)
    full, kappa = P.truth_fit_mp(dim, xk, fk, nk, xi, fi_in, order, knowns, wm, dps=dps, as_mp=True)
    with mp.workdps(dps):
        zero, one = mpf(0), mpf(1)
        beta = one - mpf(ALPHA)
        if as_mp:
            gxk[...] = zero; gxi[...] = zero
        for j in range(n):
            sysm = P._system_mp(dim, xk, nk, xi, order, knowns, wm, j)
            if sysm is None:
                continue
            no, nkj, U, C, w = sysm["no"], sysm["nk"], sysm["unknown"], sysm["C"], sysm["w"]
            low = lowered(dim, int(order[j]))
            x = P._solve_mp(sysm["A"], [[mpf(float(g[j, a])) / sysm["s"][i]] for i, a in enumerate(U)])
            y = [zero] * no
            for i, a in enumerate(U):
                y[a] = x[i][0] / sysm["s"][i]
            phi = [zero if a in sysm["dropped"] else full[j, a] for a in range(no)]
            if dim == 1:
                d = [[mpf(float(xk[j, k])) - mpf(float(xi[j]))] for k in range(nkj)]
            else:
                d = [[mpf(float(xk[j, k, m])) - mpf(float(xi[j, m])) for m in range(dim)] for k in range(nkj)]
            sk = [mp.fdot(C[k], y) for k in range(nkj)]
            rk = [mpf(float(fk[j, k])) - mp.fdot(C[k], phi) for k in range(nkj)]
            uniform = int(wm[j]) == 1
            terms = [[[] for _ in range(dim)] for _ in range(nkj)]
            if not uniform:
                d2 = [mp.fsum(v * v for v in dk) for dk in d]
                D2 = max(d2)
                kstar = d2.index(D2)                                 # the smallest index that attains the maximum, exactly
                rho = [mp.sqrt(v / D2) for v in d2]
                for k in range(nkj):
                    for m in range(dim):
                        if rho[k] != 0:
                            terms[k][m].append(-2 * beta * (one - rho[k]) * d[k][m] / (rho[k] * D2) * sk[k] * rk[k])
                for m in range(dim):
                    terms[kstar][m].extend(2 * d[kstar][m] * (beta * (one - rho[k]) * rho[k] / D2) * sk[k] * rk[k] for k in range(nkj))
            for k in range(nkj):
                for m in range(dim):
                    for a in range(no):
                        if low[m][a] >= 0:
                            dc = C[k][low[m][a]]
                            terms[k][m].append(w[k] * rk[k] * dc * y[a])
                            terms[k][m].append(-w[k] * sk[k] * dc * phi[a])
            top = zero
            tot = [zero] * dim
            for k in range(nkj):
                for m in range(dim):
                    e = mp.fsum(terms[k][m])
                    gxk[j, k, m] = e if as_mp else float(e)
                    tot[m] -= e
                    top = max(top, mp.fsum(abs(t) for t in terms[k][m]))
            for m in range(dim):
                gxi[j, m] = tot[m] if as_mp else float(tot[m])
            if top > 0:
                s_out[j] = float(top)
    return gxk, gxi, s_out, kappa


def fit_value_mp(dim, order, d, fk, fi_in, kn, uniform, g):
    """g . fi_out of ONE case as a function of its offsets d[k][m] (mpf, inside mp.workdps): plain normal equations of the unknowns, the
    knowns moved to the right-hand side, stray high mask bits dropping the last unknowns.  For difference quotients: smooth in d away from
    a tie for the farthest neighbour and from d_k = 0."""
    from mpmath import mp, mpf
    one = mpf(1)
    ex = P.exponents(dim, order)
    no, U, known, dropped = P._unknown_set(dim, order, int(kn))
    fact = [mpf(v) for v in P._FACT]
    nk = len(d)
    C = []
    for k in range(nk):
        row = []
        for e in ex:
            v = one
            for m, p in enumerate(e):
                if p:
                    v = v * d[k][m] ** p / fact[p]
            row.append(v)
        C.append(row)
    if uniform:
        w = [one] * nk
    else:
        d2 = [mp.fsum(x * x for x in dk) for dk in d]
        D2 = max(d2)
        w = [mpf(ALPHA) + (one - mpf(ALPHA)) * (one - mp.sqrt(v / D2)) ** 2 for v in d2]
    out = mp.fsum(mpf(float(g[a])) * mpf(float(fi_in[a])) for a in list(known) + list(dropped))
    if U:
        f = [mpf(float(fk[k])) - mp.fsum(C[k][a] * mpf(float(fi_in[a])) for a in known) for k in range(nk)]
        Amat = [[mp.fsum(w[k] * C[k][a] * C[k][b] for k in range(nk)) for b in U] for a in U]
        rhs = [[mp.fsum(w[k] * C[k][a] * f[k] for k in range(nk))] for a in U]
        x = P._solve_mp(Amat, rhs)
        out += mp.fsum(mpf(float(g[a])) * x[i][0] for i, a in enumerate(U))
    return out


def geometry_adjoint_ref(dim, order, xk, fk, nk, xi, fi_in, knowns, wm, g):
    """The same formula in fp64 numpy.  Returns dict(grad_xk (n, K, dim), grad_xi (n, dim), grad_fk (n, K), fi (n, no): the oracle's fit)."""
    from oracle import oracle
    n = len(nk)
    K = int(np.asarray(xk).shape[1])
    no = P._NDOF[dim][int(order)]
    ex = P.exponents(dim, int(order))
    low = lowered(dim, int(order))
    fi = np.array(fi_in, np.float64, copy=True)
    oracle.fit_many(dim, xk, fk, nk, xi, fi, None, 0, np.full(n, order, np.int32), knowns, wm)
    gxk, gxi, gfk = np.zeros((n, K, dim)), np.zeros((n, dim)), np.zeros((n, K))
    beta = 1.0 - ALPHA
    for j in range(n):
        _, U, known, dropped = P._unknown_set(dim, int(order), int(knowns[j]))
        nkj = int(nk[j])
        if not U or nkj == 0:
            continue
        d = (np.asarray(xk[j, :nkj], np.float64) - xi[j]).reshape(nkj, 1) if dim == 1 else xk[j, :nkj, :dim] - xi[j, None, :dim]
        C = np.ones((nkj, no))
        for a, e in enumerate(ex):
            for m, p in enumerate(e):
                if p:
                    C[:, a] *= d[:, m] ** p / P._FACT[p]
        d2 = d[:, 0] * d[:, 0]
        for m in range(1, dim):
            d2 = d2 + d[:, m] * d[:, m]
        uniform = int(wm[j]) == 1
        if uniform:
            w = np.ones(nkj)
        else:
            kstar = int(np.argmax(d2))                               # numpy's argmax: the first index of the largest fp64 d2
            D2 = d2[kstar]
            rho = np.sqrt(d2 / D2)
            t = 1.0 - rho
            w = ALPHA + beta * t * t
        Cu = C[:, U]
        sc = np.sqrt((w[:, None] * Cu * Cu).sum(axis=0))
        sc[sc == 0] = 1.0
        Cs = Cu / sc
        Amat = (Cs * w[:, None]).T @ Cs
        y = np.zeros(no)
        y[U] = np.linalg.solve(Amat, g[j, U] / sc) / sc
        phi = fi[j, :no].copy()
        phi[dropped] = 0.0
        s = C @ y
        r = fk[j, :nkj] - C @ phi
        e = np.zeros((nkj, dim))
        for m in range(dim):
            dcy, dcp = np.zeros(nkj), np.zeros(nkj)
            for a in range(no):
                if low[m][a] >= 0:
                    dcy += C[:, low[m][a]] * y[a]
                    dcp += C[:, low[m][a]] * phi[a]
            e[:, m] = w * (r * dcy - s * dcp)
        if not uniform:
            with np.errstate(divide="ignore", invalid="ignore"):
                coef = np.where(rho > 0, -2.0 * beta * t / (rho * D2), 0.0)
            e += (coef * s * r)[:, None] * d
            E = float(np.sum(beta * t * rho / D2 * s * r))
            e[kstar] += 2.0 * d[kstar] * E
        gxk[j, :nkj] = e
        gxi[j] = -e.sum(axis=0)
        gfk[j, :nkj] = w * s
    return dict(grad_xk=gxk, grad_xi=gxi, grad_fk=gfk, fi=fi)


def farthest_first(dim, xk, nk, xi):
    """Per case (first index of the largest fp64 d2, smallest index of the largest exact d2); d2 in fp64 as d0 d0 + d1 d1 + d2 d2 of the
    rounded offsets, exactly from the same doubles in rationals."""
    from fractions import Fraction
    n = len(nk)
    out = np.zeros((n, 2), np.int64)
    for j in range(n):
        nkj = int(nk[j])
        if nkj == 0:
            continue
        x = np.asarray(xk[j, :nkj], np.float64).reshape(nkj, -1)[:, :dim]
        c = np.asarray(xi[j], np.float64).reshape(-1)[:dim]
        d = x - c
        d2 = d[:, 0] * d[:, 0]
        for m in range(1, dim):
            d2 = d2 + d[:, m] * d[:, m]
        exact = [sum((Fraction(float(x[k, m])) - Fraction(float(c[m]))) ** 2 for m in range(dim)) for k in range(nkj)]
        out[j] = int(np.argmax(d2)), exact.index(max(exact))
    return out


# ---- the truths of the family batches, in worker processes (as _adversarial.operator_job) -------------------------------------------

FAMILIES = tuple(f for f in A.OP_FAMILIES if not f.endswith("_edge"))
EDGE_FAMILIES = tuple(f for f in A.OP_FAMILIES if f.endswith("_edge"))
SHAPES = ((2, 2, 32), (2, 3, 30), (2, 4, 64), (3, 2, 40), (1, 2, 8), (1, 4, 12))


def geometry_job(job):
    """(family, dim, order, K, n, lo, hi) -> (grad_xk, grad_xi, s, kappa) of cases lo..hi of A.op_batch with A.op_g (field 0).  A plain
    function of plain arguments: it runs in worker processes that import numpy and mpmath only."""
    family, dim, order, K, n, lo, hi = job
    b = A.op_batch(family, dim, order, K, n)
    g = A.op_g(family, dim, order, K, n)
    s = slice(lo, hi)
    return truth_geometry_adjoint_mp(dim, b["xk"][s], b["fk"][s], b["nk"][s], b["xi"][s], b["fi0"][s], b["order_a"][s], b["kn"][s],
                                     b["wm"][s], g[s])


def geometry_truths(shape, families, n=A.N_OP, step=16, workers=12):
    """family -> (grad_xk, grad_xi, s, kappa) of a shape's batches, the slices of `step` cases spread over `workers` fresh processes."""
    dim, order, K = shape
    res = A._map(geometry_job, [(f, dim, order, K, n, lo, min(lo + step, n)) for f in families for lo in range(0, n, step)], workers)
    per = (n + step - 1) // step
    return {f: tuple(np.concatenate([r[i] for r in res[q * per:(q + 1) * per]]) for i in range(4)) for q, f in enumerate(families)}
