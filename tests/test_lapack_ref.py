"""The restatement of dgetf2 / dsytf2 in tests/_lapack_ref.py (the yardstick of tests/test_gpu_lapack_edges.py) pinned
against scipy.linalg.lapack on the exact families, bit for bit, and the coverage those families promise (CPU only)."""
import numpy as np
import pytest
import scipy.linalg.lapack as SL

import _lapack_ref as R


@pytest.mark.parametrize("kind", ["ge", "sy"])
@pytest.mark.parametrize("form", list(R.FORM_SIZES))
def test_restatement_matches_lapack_bit_for_bit_on_exact_families(kind, form):
    met, later_zero = set(), False
    for n in R.FORM_SIZES[form]:
        if n > R.EXACT_NMAX or (n > 129 and kind == "ge"):
            continue                                             # (the GPU test runs those; here they only cost time)
        for scale in ((0, -1060) if kind == "ge" and n <= 65 else (0,)):
            cases = R.exact_tie_cases(kind, n, scale_exp=scale)
            assert cases, (kind, n, scale)
            for A, ex in cases:
                fp = (R.getf2 if kind == "ge" else R.sytf2)(A)
                if kind == "ge":
                    lu, piv, info = SL.dgetrf(A)
                    piv = piv + 1
                    sel = np.ones((n, n), bool)
                else:
                    lu, piv, info = SL.dsytrf(A, lower=0)
                    sel = np.triu(np.ones((n, n), bool))
                assert np.array_equal(ex["ipiv"], fp["ipiv"]) and ex["info"] == fp["info"], (kind, n, scale)
                assert np.array_equal(R.bits(R.as_float(ex["lu"])[sel]), R.bits(fp["lu"][sel])), (kind, n, scale)
                if scale == 0:                                   # (scipy's OpenBLAS getrf leaves the column of a
                    assert np.array_equal(fp["ipiv"], piv) and fp["info"] == info, (kind, n)   # subnormal pivot unscaled)
                    assert np.array_equal(R.bits(fp["lu"][sel]), R.bits(lu[sel])), (kind, n)
                assert [e for e in ex["events"]] == [e for e in fp["events"]]
                if scale == 0:
                    kinds, z = R.tie_events(kind, n, ex)
                    met |= kinds
                    later_zero |= z
    if form != "group256_global":                                # (there the GPU test adds n = 257, 300 and first-step ties)
        assert met >= R.TIE_KINDS_REQUIRED[form], (kind, form, met)
    assert later_zero, (kind, form)


def test_restatement_decisions_match_dsytrf_on_the_bunch_kaufman_families():
    met = set()
    for n in (2, 5, 8, 9, 17, 33, 64):
        rng = np.random.default_rng([13, n])
        for fam in R.BK_FAMILIES:
            for _ in range(3):
                A = R.bk_family(rng, fam, n)
                fp = R.sytf2(A)
                lu, piv, info = SL.dsytrf(A, lower=0)
                assert np.array_equal(fp["ipiv"], piv) and fp["info"] == info, (n, fam)
                iu = np.triu_indices(n)
                assert np.abs(fp["lu"][iu] - lu[iu]).max() <= 1e-10 * max(1.0, np.abs(lu[iu]).max())
                assert np.abs(R.udut(fp["lu"], fp["ipiv"]) - A).max() <= 64 * n * R.EPS * max(1.0, np.abs(A).max())
                met |= R.branches(fp["events"])
    assert met >= R.BK_BRANCHES, met


def test_restatement_nan_head_is_idamax():
    """dgetrf of a matrix with A[0, 0] = NaN keeps row 1 (nothing compares greater than a NaN head); a NaN further down
    is never chosen"""
    rng = np.random.default_rng(3)
    A = rng.uniform(-1.0, 1.0, (12, 12))
    A[0, 0] = np.nan
    assert SL.dgetrf(A)[1][0] == 0 and R.getf2(A, steps=1)["ipiv"][0] == 1
    A = rng.uniform(-1.0, 1.0, (12, 12))
    A[5, 0] = np.nan
    want = int(np.nanargmax(np.abs(A[:, 0])))
    assert SL.dgetrf(A)[1][0] == want and R.getf2(A, steps=1)["ipiv"][0] == want + 1


def test_tie_kinds_follow_the_thread_mapping():
    assert R.tie_kinds(5, 0, [1, 3], "ge") == {"lane"}
    assert R.tie_kinds(20, 3, [4, 10], "ge") == {"lanes"}
    assert R.tie_kinds(300, 2, [10, 266], "ge") == {"thread"}
    assert R.tie_kinds(300, 0, [10, 100], "ge") == {"waves"}
    assert R.tie_kinds(300, 300, [1, 257], "sy") == {"thread"}
