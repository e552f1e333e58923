"""The batched LU / Bunch-Kaufman kernels (csrc/lapack_batched.hip) on adversarial inputs, in every kernel form (lane
n <= 8, a group of 64 up to 32, a group of 256 with A in LDS up to 89 and in global memory above): singular systems
inside batches, exact ties of the pivot searches, every Bunch-Kaufman branch, power-of-two scaling, pivots below
DBL_MIN, ill-conditioned matrices, a NaN at the head of a pivot column, and batches past the launch chunk.  The
yardsticks are scipy.linalg.lapack, the plain restatement of dgetf2 / dsytf2 in tests/_lapack_ref.py, and
extended-precision solutions."""
import numpy as np
import pytest
import scipy.linalg.lapack as SL

import _lapack_ref as R
from wlsqm.utils import lapackdrivers as L

pytestmark = pytest.mark.gpu

EPS = R.EPS
FORMS = list(R.FORM_SIZES)


def fort(a):
    return np.asfortranarray(a)


def stack(mats):
    return fort(np.stack(mats, axis=2))


def raw(a):
    """the exact bits, the sign of zero included"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def dev(a):
    """a host array as a device tensor with Fortran strides (1, n, n*n) even where a dimension is 1"""
    import torch
    a = fort(a)
    t = torch.from_numpy(a)
    strides = tuple(int(np.prod(a.shape[:i])) for i in range(a.ndim))
    return torch.empty_strided(a.shape, strides, dtype=t.dtype, device="cuda").copy_(t)


def gpu_factor(kind, A3):
    """getrf_batched / sytrf_batched of a host (n, n, count) batch: (factor, ipiv, info) back on the host"""
    import torch
    from wlsqm import hip as H
    T = dev(A3)
    ipiv, info = (H.getrf_batched if kind == "ge" else H.sytrf_batched)(T)
    torch.cuda.synchronize()
    return T.cpu().numpy(), ipiv.cpu().numpy(), info.cpu().numpy()


def gpu_factor_solve(kind, A3, b2, stream):
    """gesv_batched / sysv_batched on `stream`: (factor, ipiv, info, b)"""
    import torch
    from wlsqm import hip as H
    with torch.cuda.stream(stream):
        T = dev(A3); bt = dev(b2)
        ipiv, info = (H.gesv_batched if kind == "ge" else H.sysv_batched)(T, bt)
    stream.synchronize()
    return T.cpu().numpy(), ipiv.cpu().numpy(), info.cpu().numpy(), bt.cpu().numpy()


def lapack(kind, A):
    """scipy's dgetrf (pivots made 1-based) / dsytrf (uplo 'U'): (factor, ipiv, info)"""
    if kind == "ge":
        lu, piv, info = SL.dgetrf(A)
        return lu, piv + 1, info
    return SL.dsytrf(A, lower=0)


def upper(F):
    return F[np.triu_indices(F.shape[0])]


def factor_residual(kind, A, F, ipiv):
    """max |P A - L U| / max |L| |U| (or the same of A - U D U^T) of one factor"""
    n = A.shape[0]
    if kind == "ge":
        Lf, Uf = np.tril(F, -1) + np.eye(n), np.triu(F)
        E, scale = R.lu_rows(A, ipiv) - Lf @ Uf, np.abs(Lf) @ np.abs(Uf)
    else:
        Ut, D = R.udut(F, ipiv, parts=True)
        E, scale = Ut @ D @ Ut.T - R.sym_from_upper(A), np.abs(Ut) @ np.abs(D) @ np.abs(Ut).T
    return np.abs(E).max() / max(scale.max(), 1e-300)


def regular_batch(rng, kind, n, cnt):
    A = rng.uniform(-1.0, 1.0, (n, n, cnt))
    if kind == "sy":
        A = 0.5 * (A + A.transpose(1, 0, 2))
    return fort(A)


# ---------------------------------------------------------------------------------------------------------------------
# 1. singular systems inside batches: info as LAPACK's, b bit-unchanged (dgesv / dsysv solve only when INFO = 0), the
#    factor and ipiv written, the regular neighbours bit-identical to a batch without the singular ones
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ge", "sy"])
@pytest.mark.parametrize("form", FORMS)
def test_singular_systems_keep_their_rhs(kind, form):
    import torch
    stream = torch.cuda.Stream()
    for n in R.FORM_SIZES[form]:
        rng = np.random.default_rng([11, n, kind == "sy"])
        cnt = 70 if n <= 300 else 3                              # 70: the lane form's second wave holds one too
        A0 = regular_batch(rng, kind, n, cnt)
        b0 = fort(rng.uniform(-1.0, 1.0, (n, cnt)))
        As = A0.copy(order="F")
        sing = {1: "zero_col", 2: "zero_all", 66: "zero_col"}
        sing = {k: v for k, v in sing.items() if k < cnt}
        for k, how in sing.items():
            c = (5 * k) % n
            if how == "zero_all":
                As[:, :, k] = 0.0
            else:
                As[:, c, k] = 0.0
                if kind == "sy":
                    As[c, :, k] = 0.0                            # a zero row-and-column pair
        keep = np.setdiff1d(np.arange(cnt), list(sing))
        Fc, Pc, Ic, Xc = gpu_factor_solve(kind, A0, b0, stream)
        Fs, Ps, Is, Xs = gpu_factor_solve(kind, As, b0, stream)
        for k in range(cnt) if n <= 129 else sorted(sing) + [0]:
            lu, piv, info = lapack(kind, As[:, :, k])
            assert Is[k] == info, (kind, n, k)
            if k in sing:
                assert info > 0
                assert np.array_equal(raw(Xs[:, k]), raw(b0[:, k])), (kind, n, k, "b of a singular system changed")
                assert np.array_equal(Ps[:, k], piv), (kind, n, k)
                assert np.all(np.isfinite(Fs[:, :, k]))
                assert factor_residual(kind, As[:, :, k], Fs[:, :, k], Ps[:, k]) <= 16 * n * EPS, (kind, n, k)
        assert np.array_equal(raw(Fs[:, :, keep]), raw(Fc[:, :, keep]))
        assert np.array_equal(Ps[:, keep], Pc[:, keep]) and np.array_equal(Is[keep], Ic[keep]) and np.all(Ic == 0)
        assert np.array_equal(raw(Xs[:, keep]), raw(Xc[:, keep]))
        # the host families: the batch, one matrix, one matrix with many right-hand sides (copy or in place)
        X = "general" if kind == "ge" else "symmetric"
        A = As.copy(order="F"); x = b0.copy(order="F")
        assert getattr(L, "m" + X)(A, x) == 0
        assert np.array_equal(raw(x), raw(Xs)) and np.array_equal(raw(A), raw(Fs))
        for k in sorted(sing)[:2]:
            M = As[:, :, k].copy(order="F")
            A1 = M.copy(order="F"); x1 = b0[:, k].copy()
            assert getattr(L, X)(A1, x1) == 0
            assert np.array_equal(raw(x1), raw(b0[:, k]))
            Fk, _, _ = gpu_factor(kind, M[:, :, None])
            B0 = fort(rng.uniform(-1.0, 1.0, (n, 5)))
            A1 = M.copy(order="F"); B = B0.copy(order="F")
            assert getattr(L, X + "s")(A1, B) == 0
            assert np.array_equal(raw(B), raw(B0)) and np.array_equal(raw(A1), raw(Fk[:, :, 0]))
            A1 = M.copy(order="F"); B = B0.copy(order="F")
            assert getattr(L, X + "sp")(A1, B, 2) == 0
            assert np.array_equal(raw(B), raw(B0)) and np.array_equal(raw(A1), raw(M))


# ---------------------------------------------------------------------------------------------------------------------
# 2. ties of the pivot searches, exact by construction: factor and pivots bit-identical to the restatement and to LAPACK
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ge", "sy"])
@pytest.mark.parametrize("form", FORMS)
def test_ties_are_broken_as_idamax(kind, form):
    met, later_zero = set(), False
    for n in R.FORM_SIZES[form]:
        if n <= R.EXACT_NMAX:
            cases = R.exact_tie_cases(kind, n)
            assert cases, (kind, n)
            F, P, I = gpu_factor(kind, stack([A for A, _ in cases]))
            for k, (A, ref) in enumerate(cases):
                want = R.as_float(ref["lu"])
                lu, piv, info = lapack(kind, A)
                assert np.array_equal(P[:, k], ref["ipiv"]) and np.array_equal(P[:, k], piv), (kind, n, k)
                assert I[k] == ref["info"] == info, (kind, n, k)
                if kind == "ge":
                    assert np.array_equal(R.bits(F[:, :, k]), R.bits(want)), (kind, n, k)
                    assert np.array_equal(R.bits(F[:, :, k]), R.bits(lu)), (kind, n, k)
                else:
                    assert np.array_equal(R.bits(upper(F[:, :, k])), R.bits(upper(want))), (kind, n, k)
                    assert np.array_equal(R.bits(upper(F[:, :, k])), R.bits(upper(lu))), (kind, n, k)
                    il = np.tril_indices(n, -1)
                    assert np.array_equal(raw(F[:, :, k][il]), raw(A[il]))
                kinds, z = R.tie_events(kind, n, ref)
                met |= kinds
                later_zero |= z
        # the first step alone: exact ties in random signed matrices at every distance, against LAPACK
        rng = np.random.default_rng([12, n, kind == "sy"])
        mats, wins = [], []
        for dist in R._tie_distances(rng, n - (kind == "sy")):
            A, r = R.first_step_tie_matrix(rng, kind, n, dist)
            mats.append(A); wins.append(r)
            met |= R.tie_kinds(n, 0, [r, r + dist], "ge") if kind == "ge" else R.tie_kinds(n, n, [r + 1, r + 1 + dist], "sy")
        if mats:
            F, P, I = gpu_factor(kind, stack(mats))
            for k, A in enumerate(mats):
                lu, piv, info = lapack(kind, A)
                assert np.array_equal(P[:, k], piv), (kind, n, k)
                if kind == "ge":
                    assert P[0, k] == wins[k] + 1
                else:
                    assert abs(P[n - 1, k]) == wins[k] + 1
    assert met >= R.TIE_KINDS_REQUIRED[form], (kind, form, met)
    assert later_zero, (kind, form)


# ---------------------------------------------------------------------------------------------------------------------
# 3. every Bunch-Kaufman branch in every form: pivots as dsytrf's, backward errors through the GPU's sytrs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_every_bunch_kaufman_branch(form):
    import torch
    from wlsqm import hip as H
    met = set()
    for n in R.FORM_SIZES[form]:
        rng = np.random.default_rng([13, n])
        reps = 3 if n <= 129 else 1
        fams = R.BK_FAMILIES if n <= 300 else ("normal", "zero_diag")
        mats = [R.bk_family(rng, f, n) for f in fams for _ in range(reps)]
        S = stack(mats)
        F, P, I = gpu_factor("sy", S)
        for k, A in enumerate(mats):
            lu, piv, info = SL.dsytrf(A, lower=0)
            assert np.array_equal(P[:, k], piv), (n, k)
            assert I[k] == info == 0
            if n <= 300:
                met |= R.branches(R.sytf2(A)["events"])
        # one factor per right-hand side
        b = fort(rng.uniform(-1.0, 1.0, (n, len(mats))))
        x = b.copy(order="F")
        assert L.msymmetricfactored(F.copy(order="F"), P.copy(order="F"), x) == 0
        assert np.all(R.backward_errors(S, x, b) <= 16 * n * EPS), n
        # one factor for every right-hand side (the first matrix of every family)
        for k in range(0, len(mats), reps):
            B = dev(rng.uniform(-1.0, 1.0, (n, 7)))
            B0 = B.cpu().numpy()
            H.sytrs_batched(dev(F[:, :, k:k + 1]), dev(P[:, k:k + 1]), B)
            torch.cuda.synchronize()
            be = R.backward_errors(np.repeat(S[:, :, k:k + 1], 7, 2), B.cpu().numpy(), B0)
            assert np.all(be <= 16 * n * EPS), (n, k)
    assert met >= R.BK_BRANCHES, (form, met)


# ---------------------------------------------------------------------------------------------------------------------
# 4. power-of-two scaling (exact): 2^s A factors into the same pivots, scaled U / D, unchanged multipliers; x scales by 2^-s
# ---------------------------------------------------------------------------------------------------------------------
def d_block_mask(ipiv):
    """entries of the dsytrf factor that belong to D (the rest of the upper triangle are multipliers)"""
    n = ipiv.size
    m = np.zeros((n, n), bool)
    k = n
    while k >= 1:
        if ipiv[k - 1] > 0:
            m[k - 1, k - 1] = True
            k -= 1
        else:
            m[k - 2, k - 2] = m[k - 2, k - 1] = m[k - 1, k - 1] = True
            k -= 2
    return m


@pytest.mark.parametrize("kind", ["ge", "sy"])
@pytest.mark.parametrize("form", FORMS)
def test_power_of_two_scaling_is_exact(kind, form):
    import torch
    stream = torch.cuda.Stream()
    checked = 0
    for n in R.FORM_SIZES[form]:
        rng = np.random.default_rng([14, n, kind == "sy"])
        cnt = 8 if n <= 300 else 2
        A = regular_batch(rng, kind, n, cnt)
        b = fort(rng.uniform(-1.0, 1.0, (n, cnt)))
        F, P, I, X = gpu_factor_solve(kind, A, b, stream)
        for s in (-500, 500):
            Fs, Ps, Is, Xs = gpu_factor_solve(kind, fort(np.ldexp(A, s)), b, stream)
            for k in range(cnt):
                assert np.array_equal(Ps[:, k], P[:, k]) and Is[k] == I[k] == 0, (kind, n, s, k)
                if kind == "ge":
                    scaled = np.triu(np.ones((n, n), bool))
                    region = np.ones((n, n), bool)
                else:
                    scaled = d_block_mask(P[:, k])
                    region = np.triu(np.ones((n, n), bool))
                want = np.where(scaled, np.ldexp(F[:, :, k], s), F[:, :, k])
                xw = np.ldexp(X[:, k], -s)
                tiny = lambda v: np.any((v != 0) & (np.abs(v) < R.DBL_MIN))
                if tiny(want[region]) or tiny(xw):
                    continue                                     # an expected entry would be subnormal
                assert np.array_equal(raw(Fs[:, :, k][region]), raw(want[region])), (kind, n, s, k)
                assert np.array_equal(raw(Xs[:, k]), raw(xw)), (kind, n, s, k)
                checked += 1
    assert checked >= len(R.FORM_SIZES[form]) * 2


# ---------------------------------------------------------------------------------------------------------------------
# 5. pivots below DBL_MIN: the column is divided by the pivot (its reciprocal would overflow)
# ---------------------------------------------------------------------------------------------------------------------
def lu_check_scaled_back(A, F, ipiv, cols, e):
    """F is the factor of A whose columns `cols` were multiplied by 2^-e: with those columns of A and U multiplied back
    by 2^e (exact), P A - L U must be within rounding of |L| |U|, plus the absolute rounding of subnormal arithmetic"""
    n = A.shape[0]
    Lf = np.tril(F, -1) + np.eye(n)
    Uf = np.triu(F).copy()
    Au = A.copy()
    Uf[:, cols] = np.ldexp(Uf[:, cols], e)
    Au[:, cols] = np.ldexp(Au[:, cols], e)
    E = np.abs(R.lu_rows(Au, ipiv) - Lf @ Uf)
    tol = 8 * n * EPS * (np.abs(Lf) @ np.abs(Uf)) + 8 * n * np.ldexp(1.0, -1074 + e)
    return np.all(E <= tol)


@pytest.mark.parametrize("form", FORMS)
def test_pivots_below_dbl_min_are_divided(form):
    for n in R.FORM_SIZES[form]:
        rng = np.random.default_rng([15, n])
        cnt = 4 if n <= 300 else 1
        base = rng.uniform(-1.0, 1.0, (n, n, cnt))
        for c in sorted({0, n // 2}):
            A = base.copy()
            A[:, c, :] = np.ldexp(A[:, c, :], -1030)
            A = fort(A)
            F, P, I = gpu_factor("ge", A)
            for k in range(cnt):
                # pivots from the restatement: scipy's OpenBLAS getrf leaves the column of a subnormal pivot unscaled at
                # small n (reference dgetf2 divides it), so its later pivots are not LAPACK's
                ref = R.getf2(A[:, :, k])
                assert np.array_equal(P[:, k], ref["ipiv"]) and I[k] == ref["info"] == 0, (n, c, k)
                Fk = F[:, :, k]
                assert np.all(np.isfinite(Fk)), (n, c, k)
                assert np.all(np.abs(np.tril(Fk, -1)) <= 1.0), (n, c, k)
                assert lu_check_scaled_back(A[:, :, k], Fk, P[:, k], [c], 1030), (n, c, k)
        if n <= 129:                                             # the whole matrix 2^-1060: exact cases, every op subnormal
            cases = R.exact_tie_cases("ge", n, scale_exp=-1060)
            assert cases, n
            F, P, I = gpu_factor("ge", stack([A for A, _ in cases]))
            for k, (A, ref) in enumerate(cases):
                assert np.array_equal(P[:, k], ref["ipiv"]) and I[k] == ref["info"], (n, k)
                assert np.array_equal(R.bits(F[:, :, k]), R.bits(R.as_float(ref["lu"]))), (n, k)
                assert np.all(np.isfinite(F[:, :, k])) and np.all(np.abs(np.tril(F[:, :, k], -1)) <= 1.0)
                if I[k] == 0:
                    assert lu_check_scaled_back(A, F[:, :, k], P[:, k], list(range(n)), 1060), (n, k)


# ---------------------------------------------------------------------------------------------------------------------
# 6. ill-conditioned matrices (condition numbers up to 1e12): backward error of order n eps, forward error of order
#    n cond eps against a solution refined in extended precision
# ---------------------------------------------------------------------------------------------------------------------
def ill_conditioned(rng, name, n, kind):
    i = np.arange(n)
    if name == "hilbert":                                        # Hilbert matrix lifted to a condition number ~1e11
        M = 1.0 / (i[:, None] + i[None, :] + 1.0)
        M = M + np.eye(n) * (np.abs(M).sum(axis=1).max() * 1e-11)
        if kind == "ge":
            M = M * rng.choice([-1.0, 1.0], n)[:, None]
    elif name == "graded":                                       # rows and columns graded over 4 decades each
        G = rng.uniform(-1.0, 1.0, (n, n)) + np.eye(n) * 2.0
        if kind == "sy":
            G = 0.5 * (G + G.T)
        d = 10.0 ** (-np.linspace(0.0, 4.0, n))
        M = d[:, None] * G * d[None, :]
    else:                                                        # Kahan: diag(s^i) (I - c * strict upper ones)
        s = 1e-8 ** (1.0 / max(1, n - 1))
        c = min(0.5, 2.0 / n)
        M = (s ** i)[:, None] * (np.eye(n) - c * np.triu(np.ones((n, n)), 1))
        if kind == "sy":
            M = M + M.T
    return fort(M)


def refined(A, b):
    """A x = b solved with iterative refinement, residuals in extended precision (np.longdouble)"""
    Al, bl = A.astype(np.longdouble), b.astype(np.longdouble)
    x = np.linalg.solve(A, b).astype(np.longdouble)
    for _ in range(8):
        r = bl - Al @ x
        x = x + np.linalg.solve(A, r.astype(np.float64)).astype(np.longdouble)
    return x


@pytest.mark.parametrize("kind", ["ge", "sy"])
@pytest.mark.parametrize("form", FORMS)
def test_ill_conditioned_families(kind, form):
    checked = 0
    for n in R.FORM_SIZES[form]:
        if n == 1:
            continue
        rng = np.random.default_rng([16, n, kind == "sy"])
        mats = []
        for name in ("hilbert", "graded", "kahan"):
            M = ill_conditioned(rng, name, n, kind)
            cond = np.linalg.norm(M, np.inf) * np.linalg.norm(np.linalg.inv(M), np.inf)
            if cond <= 1e12:
                mats.append((M, cond))
        A = stack([M for M, _ in mats])
        b = fort(rng.uniform(-1.0, 1.0, (n, len(mats))))
        x = b.copy(order="F")
        getattr(L, "mgeneral" if kind == "ge" else "msymmetric")(A.copy(order="F"), x)
        assert np.all(R.backward_errors(A, x, b) <= 16 * n * EPS), (kind, n)
        for k, (M, cond) in enumerate(mats):
            xr = refined(M, b[:, k])
            fe = float(np.abs(x[:, k] - xr).max() / np.abs(xr).max())
            assert fe <= 16 * n * cond * EPS, (kind, n, k, fe, cond)
            checked += 1
    assert checked >= 2 * len(R.FORM_SIZES[form]) - 2


# ---------------------------------------------------------------------------------------------------------------------
# 7. a NaN at the head of the first pivot column: idamax's answer (nothing beats a NaN head), the neighbours untouched
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ge", "sy"])
@pytest.mark.parametrize("form", FORMS)
def test_nan_head_of_the_pivot_column(kind, form):
    for n in R.FORM_SIZES[form]:
        rng = np.random.default_rng([17, n, kind == "sy"])
        cnt = 5
        A0 = regular_batch(rng, kind, n, cnt)
        An = A0.copy(order="F")
        if kind == "ge":
            An[0, 0, 2] = np.nan
        else:
            An[0, n - 1, 2] = An[n - 1, 0, 2] = np.nan                # U(1, n): the head of the first column searched
        Fc, Pc, Ic = gpu_factor(kind, A0)
        Fn, Pn, In = gpu_factor(kind, An)
        ref = (R.getf2 if kind == "ge" else R.sytf2)(An[:, :, 2], steps=1)
        if kind == "ge":
            assert Pn[0, 2] == 1 == ref["ipiv"][0], (n, Pn[:, 2])
            if n <= 12:                                          # (scipy's OpenBLAS idamax passes over a NaN head
                assert SL.dgetrf(An[:, :, 2])[1][0] == 0         # at larger n; reference idamax does not)
        else:
            assert Pn[n - 1, 2] == ref["ipiv"][n - 1], (n, Pn[:, 2], ref["ipiv"])
            if ref["ipiv"][n - 1] < 0:
                assert Pn[n - 2, 2] == ref["ipiv"][n - 2]
        keep = [0, 1, 3, 4]
        assert np.array_equal(raw(Fn[:, :, keep]), raw(Fc[:, :, keep])), n
        assert np.array_equal(Pn[:, keep], Pc[:, keep]) and np.array_equal(In[keep], Ic[keep]), n


# ---------------------------------------------------------------------------------------------------------------------
# 8. batches past the launch chunk (2^24 problems; 2^22 for the 256-thread form)
# ---------------------------------------------------------------------------------------------------------------------
def test_batches_beyond_the_launch_chunk():
    import torch
    from wlsqm import hip as H
    g = torch.Generator(device="cuda").manual_seed(18)
    C = 1 << 24

    def fortran3(n, count):
        T = torch.rand((count, n, n), dtype=torch.float64, device="cuda", generator=g)
        T.diagonal(dim1=1, dim2=2).add_(float(n))
        return T.permute(2, 1, 0)                                # (n, n, count), strides (1, n, n*n)

    def fortran2(n, count):
        return torch.rand((count, n), dtype=torch.float64, device="cuda", generator=g).t()

    probe = lambda count: sorted({k for k in (0, C - 1, C, C + 1, count - 1) if k < count})
    try:
        # gesv at n = 2 (lane form), 2^24 + 65 problems
        count = C + 65
        A = fortran3(2, count); b = fortran2(2, count)
        A1 = {k: A[:, :, k:k + 1].clone() for k in probe(count)}
        b1 = {k: b[:, k:k + 1].clone() for k in probe(count)}
        ipiv, info = H.gesv_batched(A, b)
        for k in probe(count):
            p1, i1 = H.gesv_batched(A1[k], b1[k])
            torch.cuda.synchronize()
            assert torch.equal(A[:, :, k], A1[k][:, :, 0]) and torch.equal(b[:, k], b1[k][:, 0]), k
            assert torch.equal(ipiv[:, k], p1[:, 0]) and int(info[k]) == int(i1[0]) == 0, k
        del A, b, A1, b1, ipiv, info
        # getrs / sytrs with one shared factor, 2^24 + 1 right-hand sides, in the group of 64 and of 256
        count = C + 1
        for n in (9, 33):
            F = fortran3(n, 1)
            for kind in ("ge", "sy"):
                Fk = F.clone(memory_format=torch.preserve_format)
                pv, inf = (H.getrf_batched if kind == "ge" else H.sytrf_batched)(Fk)
                b = fortran2(n, count)
                b1 = {k: b[:, k:k + 1].clone() for k in probe(count)}
                (H.getrs_batched if kind == "ge" else H.sytrs_batched)(Fk, pv, b)
                for k in probe(count):
                    (H.getrs_batched if kind == "ge" else H.sytrs_batched)(Fk, pv, b1[k])
                    torch.cuda.synchronize()
                    assert torch.equal(b[:, k], b1[k][:, 0]), (kind, n, k)
                assert bool(torch.isfinite(b[:, C - 4:C + 2]).all())
                del b, b1
            del F
    finally:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
