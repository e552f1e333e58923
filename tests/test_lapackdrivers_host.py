"""wlsqm.utils.lapackdrivers without a GPU: the public surface (names, parameter names and order), the host helpers
against numpy / scipy, and the argument checks that reject a bad layout or dtype before anything reaches the device."""
import inspect

import numpy as np
import pytest

from wlsqm.utils import lapackdrivers as L

SIGNATURES = {
    "distribute_items": ["nitems", "ntasks"],
    "copygeneral": ["O", "I"],
    "copysymmu": ["O", "I"],
    "symmetrize": ["A"],
    "msymmetrize": ["A"],
    "msymmetrizep": ["A", "ntasks"],
    "do_rescale": ["A", "algo"],
    "rescale_columns": ["A"],
    "rescale_rows": ["A"],
    "rescale_twopass": ["A"],
    "rescale_dgeequ": ["A"],
    "rescale_ruiz2001": ["A"],
    "rescale_scalgm": ["A"],
    "tridiag": ["a", "b", "c", "x"],
    "symmetric2x2": ["A", "b"],
    "symmetric": ["A", "b"],
    "symmetricfactor": ["A"],
    "symmetricfactored": ["A", "ipiv", "b"],
    "symmetrics": ["A", "b"],
    "symmetricsp": ["A", "b", "ntasks"],
    "msymmetric": ["A", "b"],
    "msymmetricp": ["A", "b", "ntasks"],
    "msymmetricfactor": ["A", "ipiv"],
    "msymmetricfactored": ["A", "ipiv", "b"],
    "msymmetricfactorp": ["A", "ipiv", "ntasks"],
    "msymmetricfactoredp": ["A", "ipiv", "b", "ntasks"],
    "general2x2": ["A", "b"],
    "general": ["A", "b"],
    "generalfactor": ["A"],
    "generalfactored": ["A", "ipiv", "b"],
    "generals": ["A", "b"],
    "generalsp": ["A", "b", "ntasks"],
    "mgeneral": ["A", "b"],
    "mgeneralp": ["A", "b", "ntasks"],
    "mgeneralfactor": ["A", "ipiv"],
    "mgeneralfactored": ["A", "ipiv", "b"],
    "mgeneralfactorp": ["A", "ipiv", "ntasks"],
    "mgeneralfactoredp": ["A", "ipiv", "b", "ntasks"],
    "svd": ["A"],
}


def F(a):
    return np.asfortranarray(a)


def test_public_names_and_signatures():
    public = sorted(n for n in dir(L) if not n.startswith("_") and n not in ("C", "B", "np", "IntEnum"))
    assert public == sorted(list(SIGNATURES) + ["ScalingAlgo"])
    assert sorted(L.__all__) == public
    for name, params in SIGNATURES.items():
        assert list(inspect.signature(getattr(L, name)).parameters) == params, name


def test_wlsqm_does_not_reexport_utils():
    import wlsqm
    assert not hasattr(wlsqm, "general") and not hasattr(wlsqm, "mgeneral")


def test_scaling_algo_members():
    assert {m.name: int(m) for m in L.ScalingAlgo} == {"ALGO_COLS_EUCL": 1, "ALGO_ROWS_EUCL": 2, "ALGO_TWOPASS": 3,
                                                        "ALGO_RUIZ2001": 4, "ALGO_SCALGM": 5, "ALGO_DGEEQU": 6}


def test_tridiag_against_dense_solve(rng):
    n = 9
    a = rng.random(n - 1); b = rng.random(n) + 3.0; c = rng.random(n - 1); x = rng.random(n)
    M = np.diag(b) + np.diag(a, -1) + np.diag(c, 1)
    want = np.linalg.solve(M, x)
    assert L.tridiag(a, b, c, x) == 0
    assert np.allclose(x, want, rtol=1e-13, atol=1e-14)


def test_svd_singular_values(rng):
    A = F(rng.random((6, 4)))
    want = np.linalg.svd(A, compute_uv=False)
    assert np.allclose(L.svd(A.copy(order="F")), want, rtol=1e-13)


def test_column_and_row_scaling_give_unit_norms(rng):
    A = F(rng.random((7, 7)))
    r, c = L.rescale_columns(A)
    assert np.allclose(np.linalg.norm(A, axis=0), 1.0, atol=1e-12)
    assert np.all(r == 1.0) and c.shape == (7,)
    A = F(rng.random((7, 5)))
    r, c = L.rescale_rows(A)
    assert np.allclose(np.linalg.norm(A, axis=1), 1.0, atol=1e-12)
    assert np.all(c == 1.0) and r.shape == (7,)


@pytest.mark.parametrize("algo", [L.ScalingAlgo.ALGO_RUIZ2001, L.ScalingAlgo.ALGO_SCALGM])
def test_iterative_scalings_keep_symmetry_and_equilibrate(rng, algo):
    A = rng.random((8, 8)); A = F(A + A.T)
    r, c = L.do_rescale(A, algo)
    assert np.allclose(A, A.T, atol=1e-12)
    if algo == L.ScalingAlgo.ALGO_RUIZ2001:
        assert np.allclose(np.abs(A).max(axis=0), 1.0, atol=1e-6)
    assert np.all(r > 0) and np.all(c > 0)


def test_twopass_and_dispatcher_agree(rng):
    A1 = F(rng.random((6, 6))); A2 = A1.copy(order="F")
    r1, c1 = L.rescale_twopass(A1)
    r2, c2 = L.do_rescale(A2, L.ScalingAlgo.ALGO_TWOPASS)
    assert np.array_equal(r1, r2) and np.array_equal(c1, c2) and np.array_equal(A1, A2)
    A3 = F(rng.random((6, 6))); A0 = A3.copy()
    r3, c3 = L.do_rescale(A3, 3)                             # a plain int works as well
    assert np.allclose(A3, A0 * r3[:, None] * c3[None, :], rtol=1e-15)


def test_dgeequ_and_unknown_algorithm(rng):
    A = F(rng.random((5, 5)))
    r, c = L.rescale_dgeequ(A)
    assert np.all(r > 0) and np.all(c > 0)
    S = F(rng.random((4, 4))); S[2, :] = 0.0
    with pytest.raises(np.linalg.LinAlgError):
        L.rescale_dgeequ(S)
    with pytest.raises(ValueError):
        L.do_rescale(F(rng.random((3, 3))), 7)


def test_copy_helpers(rng):
    I = F(rng.random((5, 5))); O = F(np.full((5, 5), -1.0))
    L.copysymmu(O, I)
    iu = np.triu_indices(5); il = np.tril_indices(5, -1)
    assert np.array_equal(O[iu], I[iu]) and np.all(O[il] == -1.0)
    O2 = F(np.zeros((5, 5)))
    L.copygeneral(O2, I)
    assert np.array_equal(O2, I)


def test_symmetrize_formula(rng):
    A = F(rng.random((4, 4, 3))); A0 = A.copy()
    L.msymmetrize(A)
    assert np.array_equal(A, 0.5 * (A0 + A0.transpose(1, 0, 2)))
    B2 = F(rng.random((5, 5))); B0 = B2.copy()
    L.symmetrize(B2)
    assert np.array_equal(B2, 0.5 * (B0 + B0.T))
    C3 = A0.copy(order="F")
    L.msymmetrizep(C3, 4)
    assert np.array_equal(C3, A)


def test_small_direct_solvers(rng):
    A = F(rng.random((2, 2)) + np.eye(2)); b = rng.random(2); want = np.linalg.solve(A, b)
    assert L.general2x2(A, b) == 0 and np.allclose(b, want, rtol=1e-13)
    S = rng.random((2, 2)); S = F(S + S.T + 2 * np.eye(2)); b = rng.random(2); want = np.linalg.solve(S, b)
    assert L.symmetric2x2(S, b) == 0 and np.allclose(b, want, rtol=1e-13)


@pytest.mark.parametrize("nitems,ntasks", [(10, 3), (3, 3), (2, 5), (0, 4), (1000, 7)])
def test_distribute_items_covers_every_item_once(nitems, ntasks):
    sizes, bases = L.distribute_items(nitems, ntasks)
    assert sizes.dtype == np.int32 and bases.dtype == np.int32 and len(sizes) == ntasks
    covered = np.concatenate([np.arange(b, b + s) for s, b in zip(sizes, bases)] + [np.zeros(0, int)])
    assert np.array_equal(np.sort(covered), np.arange(nitems))
    assert sizes.max() - sizes[sizes > 0].min() <= 1 if nitems else True


def test_layout_and_dtype_errors_before_the_device():
    n, k = 4, 3
    A = F(np.random.default_rng(0).random((n, n, k))); b = F(np.zeros((n, k)))
    ipiv = np.zeros((n, k), dtype=np.intc, order="F")
    with pytest.raises(ValueError):
        L.mgeneral(np.ascontiguousarray(A), b)                  # C order
    with pytest.raises(ValueError):
        L.mgeneral(A, b.astype(np.float32, order="F"))           # float32 b
    with pytest.raises(ValueError):
        L.mgeneralfactor(A, ipiv.astype(np.int64, order="F"))   # int64 ipiv
    with pytest.raises(ValueError):
        L.mgeneral(A, F(np.zeros((n, k + 1))))                   # shape mismatch
    with pytest.raises(ValueError):
        L.msymmetricfactored(A, F(np.zeros((n + 1, k), dtype=np.intc)), b)
    with pytest.raises(ValueError):
        L.general(F(np.zeros((3, 4))), np.zeros(3))             # not square
    with pytest.raises(ValueError):
        L.generalfactored(A[:, :, 0].copy(order="F"), np.zeros(n, dtype=np.int64), np.zeros(n))
    with pytest.raises(ValueError):
        L.symmetric(A[:, :, 0].copy(order="F"), np.zeros((n, 1)))   # rank-2 b for a rank-1 argument
    with pytest.raises(ValueError):
        L.mgeneralp(A, b, 0)                                    # ntasks < 1
    with pytest.raises(ValueError):
        L.symmetricsp(A[:, :, 0].copy(order="F"), F(np.zeros((n, 2))), 0)
