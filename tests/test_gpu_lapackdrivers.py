"""wlsqm.utils.lapackdrivers and wlsqm.hip.*_batched on the GPU against scipy.linalg.lapack, matrix by matrix: dgetrf /
dsytrf pivots exactly, factors and solutions within rounding, across every boundary of the kernel forms (lane form n <= 8,
one workgroup of 64 threads up to 32, 256 threads above, the matrix in LDS up to 89 and in global memory above)."""
import numpy as np
import pytest
import scipy.linalg.lapack as SL

from wlsqm.utils import lapackdrivers as L

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SIZES = list(range(1, 71)) + [88, 89, 90, 91, 100, 128, 129, 200, 300]


def counts(n):
    return [1, 63, 65, max(16, min(2000, 400000 // (n * n)))]


def fort(a):
    return np.asfortranarray(a)


def backward_errors(A, x, b):
    """normwise backward error of every system A[:, :, k] x[:, k] = b[:, k] (inf norms)"""
    r = np.einsum("ijk,jk->ik", A, x) - b
    return np.abs(r).max(axis=0) / (np.abs(A).sum(axis=1).max(axis=0) * np.abs(x).max(axis=0) + np.abs(b).max(axis=0))


def amplification(M):
    """max(1, condition number), capped: how much a rounding difference in the factorization may grow"""
    with np.errstate(all="ignore"):
        c = np.linalg.cond(M)
    return float(min(max(1.0, c if np.isfinite(c) else 1e12), 1e12))


def sym_from_upper(A):
    U = np.triu(np.moveaxis(A, 2, 0))
    S = U + np.transpose(np.triu(U, 1), (0, 2, 1))
    return np.moveaxis(S, 0, 2)


def random_symmetric(rng, n, cnt, lower_fill=np.nan):
    """the reference example's matrices (uniform [0, 1), symmetrized); the strict lower triangle holds `lower_fill`"""
    A = rng.random((n, n, cnt))
    A = 0.5 * (A + A.transpose(1, 0, 2))
    il = np.tril_indices(n, -1)
    A[il[0], il[1], :] = lower_fill
    return fort(A)


@pytest.mark.parametrize("n", SIZES)
def test_getrf_matches_dgetrf(n):
    rng = np.random.default_rng(1000 + n)
    for cnt in counts(n):
        A0 = rng.random((n, n, cnt))
        if cnt > 2:                                  # one exactly singular matrix: a zero column
            A0[:, rng.integers(n), cnt // 2] = 0.0
        A0 = fort(A0)
        A = A0.copy(order="F")
        ipiv = np.empty((n, cnt), dtype=np.intc, order="F")
        assert L.mgeneralfactor(A, ipiv) == 0
        b = fort(rng.random((n, cnt)))
        for k in range(cnt):
            lu, piv, info = SL.dgetrf(A0[:, :, k])
            assert np.array_equal(ipiv[:, k], piv + 1), (n, cnt, k)
            # rounding differences of the two orders of operations are amplified in the trailing entries of an
            # ill-conditioned matrix: the tolerance grows with the condition number (pivots must match exactly anyway)
            tol = 64 * n * EPS * max(1.0, np.abs(lu).max()) * amplification(A0[:, :, k])
            assert np.abs(A[:, :, k] - lu).max() <= tol, (n, cnt, k)
            if info == 0:
                # the GPU's factor through scipy's dgetrs
                x, _ = SL.dgetrs(A[:, :, k], ipiv[:, k] - 1, b[:, k])
                assert backward_errors(A0[:, :, k:k + 1], x[:, None], b[:, k:k + 1])[0] <= 8 * n * EPS
        # scipy's factors through the GPU's getrs
        if cnt > 1:
            F = np.empty_like(A0); P = np.empty_like(ipiv); ok = np.ones(cnt, bool)
            for k in range(cnt):
                lu, piv, info = SL.dgetrf(A0[:, :, k])
                F[:, :, k] = lu; P[:, k] = piv + 1; ok[k] = info == 0
            x = b.copy(order="F")
            assert L.mgeneralfactored(F, P, x) == 0
            assert np.all(backward_errors(A0[:, :, ok], x[:, ok], b[:, ok]) <= 8 * n * EPS)


def test_getrf_info_matches_dgetrf_and_singular_neighbours_are_unaffected():
    from wlsqm import hip as H
    import torch
    rng = np.random.default_rng(7)
    for n in (6, 20, 100):
        cnt = 200
        A0 = fort(rng.random((n, n, cnt)))
        Asing = A0.copy(order="F")
        Asing[:, 3, 50] = 0.0
        Asing[:, :, 51] = 0.0
        infos = []
        outs = []
        for M in (A0, Asing):
            T = torch.from_numpy(M.copy(order="F")).cuda()
            ipiv, info = H.getrf_batched(T)
            torch.cuda.synchronize()
            infos.append(info.cpu().numpy()); outs.append((T.cpu().numpy(), ipiv.cpu().numpy()))
        for k in (50, 51):
            assert infos[1][k] == SL.dgetrf(Asing[:, :, k])[2] and infos[1][k] > 0
        keep = np.setdiff1d(np.arange(cnt), [50, 51])
        assert np.all(infos[0] == 0) and np.all(infos[1][keep] == 0)
        assert np.array_equal(outs[0][0][:, :, keep], outs[1][0][:, :, keep])
        assert np.array_equal(outs[0][1][:, keep], outs[1][1][:, keep])


@pytest.mark.parametrize("n", SIZES)
def test_sytrf_matches_dsytrf(n):
    rng = np.random.default_rng(2000 + n)
    two_by_two = 0
    for cnt in counts(n):
        A0 = random_symmetric(rng, n, cnt)
        S = sym_from_upper(A0)
        A = A0.copy(order="F")
        ipiv = np.empty((n, cnt), dtype=np.intc, order="F")
        assert L.msymmetricfactor(A, ipiv) == 0
        il = np.tril_indices(n, -1)
        # the strict lower triangle is bit-unchanged (NaN in, the same NaN out)
        assert np.array_equal(A[il[0], il[1], :].view(np.int64), A0[il[0], il[1], :].view(np.int64))
        iu = np.triu_indices(n)
        b = fort(rng.random((n, cnt)))
        F = np.empty_like(A0); P = np.empty_like(ipiv)
        for k in range(cnt):
            lu, piv, info = SL.dsytrf(S[:, :, k], lower=0)
            assert np.array_equal(ipiv[:, k], piv), (n, cnt, k)
            two_by_two += int((piv < 0).any())
            tol = 64 * n * EPS * max(1.0, np.abs(lu[iu]).max()) * amplification(S[:, :, k])
            assert np.abs(A[:, :, k][iu] - lu[iu]).max() <= tol, (n, cnt, k)
            Fu = np.triu(A[:, :, k])
            x, _ = SL.dsytrs(Fu, ipiv[:, k], b[:, k:k + 1], lower=0)
            assert backward_errors(S[:, :, k:k + 1], x, b[:, k:k + 1])[0] <= 16 * n * EPS
            F[:, :, k] = lu; P[:, k] = piv
        # scipy's factors through the GPU's sytrs
        x = b.copy(order="F")
        assert L.msymmetricfactored(F, P, x) == 0
        assert np.all(backward_errors(S, x, b) <= 16 * n * EPS)
    if n >= 6:
        assert two_by_two > 0, "the test set has no 2x2 pivots"


def test_every_solver_family():
    rng = np.random.default_rng(3)
    for n in (2, 3, 6, 8, 9, 20, 33, 64, 100):
        cnt = 300
        A0 = fort(rng.random((n, n, cnt)))
        S0 = fort(0.5 * (A0 + A0.transpose(1, 0, 2)))
        b0 = fort(rng.random((n, cnt)))
        ref_ge = np.linalg.solve(np.moveaxis(A0, 2, 0), b0.T[:, :, None])[:, :, 0].T
        ref_sy = np.linalg.solve(np.moveaxis(S0, 2, 0), b0.T[:, :, None])[:, :, 0].T
        cond_ge = np.linalg.cond(np.moveaxis(A0, 2, 0)); cond_sy = np.linalg.cond(np.moveaxis(S0, 2, 0))

        def check(x, M, ref, cond):
            assert np.all(backward_errors(M, x, b0) <= 16 * n * EPS)
            rel = np.abs(x - ref).max(axis=0) / np.abs(ref).max(axis=0)
            assert np.all(rel <= 1e3 * n * EPS * cond)

        for kind, M0, ref, cond in (("general", A0, ref_ge, cond_ge), ("symmetric", S0, ref_sy, cond_sy)):
            f = lambda name: getattr(L, name.replace("X", kind))
            # m-families
            for name, extra in (("mX", ()), ("mXp", (4,))):
                A = M0.copy(order="F"); x = b0.copy(order="F")
                assert f(name)(A, x, *extra) == 0
                check(x, M0, ref, cond)
                assert not np.array_equal(A, M0)               # A holds the factor
            for fac, sol, extra in (("mXfactor", "mXfactored", ()), ("mXfactorp", "mXfactoredp", (4,))):
                A = M0.copy(order="F"); x = b0.copy(order="F")
                ipiv = np.empty((n, cnt), dtype=np.intc, order="F")
                assert f(fac)(A, ipiv, *extra) == 0
                assert f(sol)(A, ipiv, x, *extra) == 0
                check(x, M0, ref, cond)
            # single matrix, one and many right-hand sides
            M1 = M0[:, :, 0].copy(order="F")
            xs = b0.copy(order="F")
            ref1 = np.linalg.solve(M1, b0)
            A = M1.copy(order="F")
            assert f("Xs")(A, xs) == 0
            assert not np.array_equal(A, M1)
            assert np.all(backward_errors(np.repeat(M1[:, :, None], cnt, 2), xs, b0) <= 16 * n * EPS)
            assert np.abs(xs - ref1).max() <= 1e3 * n * EPS * cond[0] * np.abs(ref1).max()
            A = M1.copy(order="F"); xsp = b0.copy(order="F")
            assert f("Xsp")(A, xsp, 3) == 0
            assert np.array_equal(A, M1)                        # the parallel form leaves A alone, as the reference does
            assert np.array_equal(xsp, xs)
            A = M1.copy(order="F"); x1 = b0[:, 0].copy()
            assert f("X")(A, x1) == 0
            assert np.abs(x1 - ref1[:, 0]).max() <= 1e3 * n * EPS * cond[0] * np.abs(ref1).max()
            A = M1.copy(order="F"); x2 = b0[:, 0].copy()
            ipiv = f("Xfactor")(A)
            assert ipiv.dtype == np.intc and ipiv.shape == (n,)
            assert f("Xfactored")(A, ipiv, x2) == 0
            assert np.all(backward_errors(M1[:, :, None], x2[:, None], b0[:, :1]) <= 16 * n * EPS)


def test_general_and_mgeneral_and_device_path_give_the_same_bits():
    import torch
    from wlsqm import hip as H
    rng = np.random.default_rng(11)
    for n, big in ((6, 100000), (20, 2000)):
        A0 = fort(rng.random((n, n, big))); b0 = fort(rng.random((n, big)))
        A = A0.copy(order="F"); x = b0.copy(order="F")
        L.mgeneral(A, x)
        A2 = A0.copy(order="F"); x2 = b0.copy(order="F")
        L.mgeneral(A2, x2)
        assert np.array_equal(A, A2) and np.array_equal(x, x2)            # two runs
        # position 777 of the big batch == a batch of one == general()
        k = 777
        A1 = A0[:, :, k:k + 1].copy(order="F"); x1 = b0[:, k:k + 1].copy(order="F")
        L.mgeneral(A1, x1)
        assert np.array_equal(A1[:, :, 0], A[:, :, k]) and np.array_equal(x1[:, 0], x[:, k])
        Ag = A0[:, :, k].copy(order="F"); xg = b0[:, k].copy()
        L.general(Ag, xg)
        assert np.array_equal(Ag, A[:, :, k]) and np.array_equal(xg, x[:, k])
        # wlsqm.hip on a non-default stream, in place
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            T = torch.from_numpy(A0).cuda(); bt = torch.from_numpy(b0).cuda()
            ipiv, info = H.gesv_batched(T, bt)
        s.synchronize()
        assert np.array_equal(T.cpu().numpy(), A) and np.array_equal(bt.cpu().numpy(), x)
        assert int(info.abs().max()) == 0
        # symmetric: host vs device
        m = min(3000, big)
        S0 = random_symmetric(rng, n, m, lower_fill=0.25)
        Sa = S0.copy(order="F"); ys = b0[:, :m].copy(order="F")
        L.msymmetric(Sa, ys)
        with torch.cuda.stream(s):
            T = torch.from_numpy(S0).cuda(); bt = torch.from_numpy(b0[:, :m].copy(order="F")).cuda()
            H.sysv_batched(T, bt, stream=s.cuda_stream)
        s.synchronize()
        assert np.array_equal(T.cpu().numpy(), Sa) and np.array_equal(bt.cpu().numpy(), ys)


def test_device_entry_points_factor_solve_and_symmetrize():
    import torch
    from wlsqm import hip as H
    rng = np.random.default_rng(12)
    n, cnt = 5, 1000
    A0 = fort(rng.random((n, n, cnt)))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        T = torch.from_numpy(A0).cuda()
        H.symmetrize_batched(T)
        Ssym = T.clone(memory_format=torch.preserve_format)
        ipiv, info = H.sytrf_batched(T)
        b = torch.from_numpy(fort(rng.random((n, cnt)))).cuda(); b0 = b.clone()
        H.sytrs_batched(T, ipiv, b)
    s.synchronize()
    S = Ssym.cpu().numpy()
    expect = A0.copy(order="F"); L.msymmetrize(expect)
    assert np.array_equal(S, expect)
    assert np.all(backward_errors(S, b.cpu().numpy(), b0.cpu().numpy()) <= 16 * n * EPS)
    # one factor for every right-hand side (A (n, n, 1))
    T1 = torch.from_numpy(A0[:, :, :1].copy(order="F")).cuda()
    p1, _ = H.getrf_batched(T1)
    bb = torch.from_numpy(fort(rng.random((n, 300)))).cuda(); bb0 = bb.clone()
    H.getrs_batched(T1, p1, bb)
    torch.cuda.synchronize()
    assert np.all(backward_errors(np.repeat(A0[:, :, :1], 300, 2), bb.cpu().numpy(), bb0.cpu().numpy()) <= 16 * n * EPS)
    with pytest.raises(ValueError):
        H.getrf_batched(torch.from_numpy(np.ascontiguousarray(A0)).cuda())


def test_host_path_streams_batches_larger_than_one_staging_chunk():
    import torch
    from wlsqm import hip as H
    rng = np.random.default_rng(13)
    n, cnt = 6, 200000                                 # 57.6 MB of matrices: two 32 MB staging chunks
    A0 = fort(rng.random((n, n, cnt))); b0 = fort(rng.random((n, cnt)))
    A = A0.copy(order="F"); x = b0.copy(order="F")
    assert L.mgeneralp(A, x, 8) == 0
    assert np.all(backward_errors(A0, x, b0) <= 64 * n * EPS)
    T = torch.from_numpy(A0).cuda(); bt = torch.from_numpy(b0).cuda()
    H.gesv_batched(T, bt)
    torch.cuda.synchronize()
    assert np.array_equal(T.cpu().numpy(), A) and np.array_equal(bt.cpu().numpy(), x)


def test_reference_example_checks():
    """the reference example's first check in our own words, then its size sweep through the batched families"""
    rng = np.random.default_rng(5)
    A = rng.random((5, 5)); A = fort(0.5 * (A + A.T)); b = rng.random(5)
    xn = np.linalg.solve(A, b)
    xg = b.copy(); L.general(A.copy(order="F"), xg)
    xs = b.copy(); L.symmetric(A.copy(order="F"), xs)
    assert np.abs(xg - xn).max() < 1e-10 and np.abs(xs - xn).max() < 1e-10
    for n in (3, 5, 10, 20, 35, 60, 100, 200, 300):
        cnt = int(min(1e6 / n, 2e7 / (n * n)))
        A0 = rng.random((n, n, cnt)); A0 = fort(0.5 * (A0 + A0.transpose(1, 0, 2)))
        b0 = fort(rng.random((n, cnt)))
        for name in ("mgeneralp", "msymmetricp", "pair_general", "pair_symmetric"):
            A = A0.copy(order="F"); x = b0.copy(order="F")
            if name.startswith("pair"):
                kind = name.split("_")[1]
                ipiv = np.empty((n, cnt), dtype=np.intc, order="F")
                getattr(L, "m%sfactorp" % kind)(A, ipiv, 4)
                getattr(L, "m%sfactoredp" % kind)(A, ipiv, x, 4)
            else:
                getattr(L, name)(A, x, 4)
            be = backward_errors(A0, x, b0)
            assert np.all(be <= 64 * n * EPS), (name, n, be.max())
