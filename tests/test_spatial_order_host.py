"""The Morton order's statement (tests/_order_ref.py) against integer truths, and what wlsqm.hip.SpatialOrder refuses before it touches a
device.  No GPU."""
import numpy as np
import pytest

import _krylov_ref as KR
import _order_ref as O
import _stencil_ref as R


def test_lattice_cases_cover_every_origin_and_the_extreme_shifts():
    cases = O.lattice_cases()
    for dim in (2, 3):
        mine = [(o, s) for d, _, o, s, f in cases if d == dim and f is None]
        assert {o for o, _ in mine} == set(O.ORIGINS)
        assert {s for _, s in mine} >= {min(O.SHIFTS), max(O.SHIFTS)}


@pytest.mark.parametrize("dim,p,origin,s,flat", O.lattice_cases())
def test_statement_meets_the_integer_truth_on_lattices(dim, p, origin, s, flat):
    rng = np.random.default_rng([5, dim, p, s + 1000])
    S, J = O.lattice(dim, p, origin, s, rng=rng, flat=flat)
    B = O.BITS[dim]
    lo, hi = O.box(S)
    q = O.cells(S, lo, hi, B)
    want = O.lattice_cells(J, p, B)
    assert np.array_equal(q, want)
    assert (want.max(axis=0)[[m for m in range(dim) if m != flat]] == 2 ** B - 1).all()          # the upper face is clamped
    key, perm, inverse = O.order(S)
    # the key of the integers, bit by bit, in pure Python
    slow = [sum(((int(v) >> b) & 1) << (b * dim + m) for m, v in enumerate(row) for b in range(B)) for row in want]
    assert key.tolist() == sorted(slow) and [slow[i] for i in perm] == key.tolist()
    assert np.array_equal(inverse[perm], np.arange(len(perm)))
    assert 0 <= int(key.min()) and int(key.max()) < 2 ** 63
    ties = key[1:] == key[:-1]
    assert (perm[1:][ties] > perm[:-1][ties]).all()


def test_coincident_points_and_duplicates_tie_by_index():
    for dim in (1, 2, 3):
        S = np.full((37, dim), 0.625)
        key, perm, inverse = O.order(S if dim > 1 else S[:, 0])
        assert np.array_equal(perm, np.arange(37)) and np.array_equal(inverse, np.arange(37))
        assert (key == key[0]).all()
    rng = np.random.default_rng(3)
    for dim in (2, 3):
        base = rng.random((50, dim))
        S = base[rng.integers(0, 50, 400)]
        key, perm, _ = O.order(S)
        assert (np.diff(key) >= 0).all()
        ties = key[1:] == key[:-1]
        assert ties.sum() >= 300 and (perm[1:][ties] > perm[:-1][ties]).all()


def test_one_dimension_is_the_exact_order_of_the_doubles():
    tiny = np.float64(5e-324)
    x = np.array([0.0, -0.0, 1.0, -1.0, tiny, -tiny, 3 * tiny, -3 * tiny, 2.2250738585072014e-308, -2.2250738585072014e-308, 1e300, -1e300,
                  -0.0, 0.0, 7.5, 7.5, -7.5, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), np.nextafter(-1.0, 0.0), np.nextafter(-1.0, -2.0)])
    rng = np.random.default_rng(11)
    x = np.concatenate([x, rng.standard_normal(500), -rng.random(200) * 1e-310, rng.random(200) * 1e-310])
    x = x[rng.permutation(len(x))]
    key, perm, inverse = O.order(x)
    assert np.array_equal(perm, np.argsort(x + 0.0, kind="stable"))          # numpy's sort of doubles puts -0.0 and +0.0 level too
    assert (np.diff(x[perm]) >= 0).all()
    k = O.keys(x)
    assert np.array_equal(k[x == 0.0], np.zeros((x == 0.0).sum(), np.int64))
    a, b = rng.integers(0, len(x), 4000), rng.integers(0, len(x), 4000)
    assert np.array_equal(k[a] < k[b], x[a] < x[b]) and np.array_equal(k[a] == k[b], x[a] == x[b])


@pytest.mark.parametrize("scale", [1.0, 1e-300, 1e150])
def test_monotone_per_axis(scale):
    rng = np.random.default_rng([19, int(np.log10(scale)) + 1000])
    x = np.sort(rng.standard_normal(100000)) * scale
    for B in (31, 21):
        q = O.cells(x, [x[0]], [x[-1]], B)[:, 0]
        assert (np.diff(q) >= 0).all() and q[0] == 0 and q[-1] == 2 ** B - 1
    k = O.keys(x)                                            # 1D: the whole int64 range, so compared, not subtracted
    assert (k[1:] >= k[:-1]).all()


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_scaling_by_a_power_of_two_keeps_the_permutation_and_keys_stay_below_2_63(dim):
    rng = np.random.default_rng([7, dim])
    S = rng.standard_normal((3000, dim)) * 10.0 - 3.0
    S = S[:, 0] if dim == 1 else S
    key, perm, _ = O.order(S)
    assert 0 <= int(key.min()) if dim > 1 else True
    assert int(key.max()) < 2 ** 63
    for e in (40, -40):
        k2, p2, _ = O.order(np.ldexp(S, e))
        assert np.array_equal(p2, perm)
        if dim > 1:
            assert np.array_equal(k2, key)


def test_keys_of_other_points_clamp_and_nan_is_largest():
    rng = np.random.default_rng(23)
    for dim in (1, 2, 3):
        S = rng.random((200, dim))
        lo, hi = O.box(S)
        X = rng.random((50, dim)) * 3.0 - 1.0
        clamped = np.clip(X, lo, hi)
        assert np.array_equal(O.keys(X, lo, hi), O.keys(clamped, lo, hi))
        X[7, dim - 1] = np.nan
        X[9] = np.inf
        X[11] = -np.inf
        k = O.keys(X, lo, hi)
        assert k[7] == O.LARGEST[dim] and k[9] == O.keys(hi[None, :], lo, hi)[0] and k[11] == O.keys(lo[None, :], lo, hi)[0]
        assert (np.delete(k, 7) <= k[9]).all()


@pytest.mark.parametrize("n,K", [(1, 4), (130, 9), (300, 12)])
def test_relabel_is_the_permuted_matrix(n, K):
    """P M P^T of a random square structure equals the dense matrix of the relabelled lists, entry for entry."""
    st = KR.square_structure(n, K, seed=31)
    rows = R.rows_of(st["hoods"], st["nk"], st["slots"], st["own"], st["own_mask"], st["pts"])
    M = R.dense(rows, n, 0)
    rng = np.random.default_rng([n, K])
    _, perm, inverse = O.order(rng.random((n, 2)))
    hoods2, bad = O.relabel(st["hoods"], st["nk"], inverse, row_perm=perm)
    assert bad == 0                                                       # the -1 / npoints padding of the structure is not live
    nk2 = st["nk"][perm]
    pad = np.arange(K)[None, :] >= nk2[:, None]
    assert np.array_equal(hoods2[pad], np.broadcast_to(np.arange(n)[:, None], (n, K))[pad])      # the row's own new number
    rows2 = R.rows_of(hoods2, nk2, st["slots"][:, perm], st["own"][:, perm], st["own_mask"][perm], np.arange(n))
    assert np.array_equal(R.dense(rows2, n, 0), O.permuted_dense(M, perm))
    # entry order inside a row is kept
    for i in (0, n // 2, n - 1):
        assert [c for c, _ in rows2[i]] == [int(inverse[c]) for c, _ in rows[perm[i]]]
        assert [v[0] for _, v in rows2[i]] == [v[0] for _, v in rows[perm[i]]]


def test_relabel_counts_what_names_no_point():
    rng = np.random.default_rng(41)
    n, K = 60, 5
    hoods = rng.integers(0, n, (n, K)).astype(np.int32)
    nk = rng.integers(1, K + 1, n).astype(np.int32)
    nk[[3, 10, 20]] = K
    _, perm, inverse = O.order(rng.random((n, 3)))
    hoods[3, 1], hoods[10, 0], hoods[20, K - 1] = n, -1, 2 ** 31 - 1
    hoods[5, K - 1], nk[5] = n + 7, K - 1                                 # padding: not looked at
    out, bad = O.relabel(hoods, nk, inverse, row_perm=perm)
    assert bad == 3
    assert out[inverse[3], 1] == -1 and out[inverse[10], 0] == -1 and out[inverse[20], K - 1] == -1 and (out == -1).sum() == 3
    assert out[inverse[5], K - 1] == inverse[5]
    # without moving rows: the padding is what the caller names
    out, bad = O.relabel(hoods, nk, inverse, own=np.full(n, -1))
    assert bad == 3 and out[5, K - 1] == -1 and out[3, 0] == inverse[hoods[3, 0]]


ASSERTED = ("2D-tau1-n130", "3D-tau0.25-n1000")
PRINTED = ("2D-dirichlet-n1000", "2D-dirichlet-n130", "3D-dirichlet-n1000", "2D-tau0.25-n1000")


@pytest.mark.parametrize("name", ASSERTED + PRINTED)
def test_rehearsal_the_solver_gains_from_the_order(name):
    """Block-16 BiCGSTAB on the systems of tests/_krylov_ref.py, as given (random order) and as P M P^T: the reordered count is at most
    0.75 of the as-given one on the two asserted systems (the CPU ratios are 0.39 and 0.58); the others are printed."""
    given, reordered, searched = O.rehearsal(name)
    print("%-22s as given %3d   reordered %3d   searched again on the sorted table %3d" % (name, given, reordered, searched))
    if name in ASSERTED:
        assert reordered <= 0.75 * given, (name, given, reordered)


def test_argument_refusals_before_any_device():
    import torch
    from _device_helpers import OnDevice
    import wlsqm.hip as H
    assert "SpatialOrder" in H.__all__
    with pytest.raises(ValueError, match=r"S must be \(npoints,\) or \(npoints, dim\) with dim 1\.\.3"):
        H.SpatialOrder(torch.zeros((5, 4), dtype=torch.float64))
    with pytest.raises(ValueError, match=r"S must be \(npoints,\) or \(npoints, dim\) with dim 1\.\.3"):
        H.SpatialOrder(torch.zeros((5, 2, 2), dtype=torch.float64))
    with pytest.raises(ValueError, match="Buffer dtype mismatch, expected 'float64'"):
        H.SpatialOrder(torch.zeros((5, 2), dtype=torch.float32))
    with pytest.raises(ValueError, match="argument S must be a device"):
        H.SpatialOrder(torch.zeros((5, 2), dtype=torch.float64))
    with pytest.raises(ValueError, match="argument S must be a device"):
        H.SpatialOrder(np.zeros((5, 2)))
    with pytest.raises(ValueError, match="S must be contiguous"):
        H.SpatialOrder(OnDevice(torch.zeros((6, 4), dtype=torch.float64)[:, :2]))
    with pytest.raises(ValueError, match="npoints must be >= 1"):
        H.SpatialOrder(OnDevice(torch.zeros((0, 2), dtype=torch.float64)))
