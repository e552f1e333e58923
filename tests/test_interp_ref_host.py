"""CPU side of the interpolation truth (tests/_interp_ref.py): the geometry is what tests/test_gpu_interp_truth.py takes it for, and an
fp64 replay of the kernels' arithmetic stays under half of the derived bounds against the long-double truth.  No device."""
import numpy as np
import pytest

import _interp_ref as R


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_geometry_is_what_the_gpu_test_takes_it_for(dim):
    g = R.geometry(dim)
    assert g["X"].shape == (R.NX, dim) and R.NX == 337 and R.NX % 64 not in (0, 63) and g["n"] == 1500
    assert set(g["order"].tolist()) == set(range(R.TOP[dim] + 1))
    assert g["edge"].sum() <= 0.001 * R.NX                       # the cap on points the ball search may decide either way
    assert g["empty"].sum() >= 20 and (~g["empty"]).sum() >= 100
    outside = (g["X"].min(axis=1) < 0.0) | (g["X"].max(axis=1) > 1.0)
    assert outside.sum() >= 20 and (outside & ~g["empty"]).any()
    assert g["nearest_gap"].min() > 1e-9                         # no point is within rounding of equidistant from two origins
    length = np.array([len(L) for L in g["lists"]])
    assert length.max() >= 8 and ((length > 0) & (length <= 3)).any()
    # the last points sit just inside a sphere: their centre is in the list, at a weight below 1e-5
    for m, c in zip(range(R.NX - R.NEAR_SPHERE, R.NX), g["centre"]):
        assert c in g["lists"][m]
        assert 0.0 < (1.0 - np.sqrt(((g["X"][m] - g["S"][c]) ** 2).sum()) / g["r"]) ** 2 < 1e-5
    assert (g["given"][::2] == g["nearest"][::2]).all() and (g["given"][1::2] != g["nearest"][1::2]).sum() > 100


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_fp64_replay_stays_under_half_of_the_bounds(dim):
    """Every diff 0 .. max_no + 1, nearest (the nearest model and the given I) and continuous; zeros and NaNs sit exactly where the
    truth has them."""
    g = R.geometry(dim)
    S, fi, order, X, r, lists = g["S"], g["fi_random"], g["order"], g["X"], g["r"], g["lists"]
    worst_n, worst_c = 0.0, 0.0
    for diff in range(g["max_no"] + 2):
        for I in (g["nearest"], g["given"]):
            T = R.truth_interpolate(dim, S, fi, order, X, diff, I=I)
            got = R.replay_interpolate(dim, S, fi, order, X, diff, I=I)
            bound = R.nearest_bound(dim, S, fi, order, X, diff, I)
            gone = diff >= g["no"][I]
            assert (T[gone] == 0).all() and (got[gone] == 0.0).all() and (bound[gone] == 0.0).all()
            assert gone.all() == (diff >= g["max_no"])
            err = np.abs((got - T).astype(np.float64))
            assert (err <= 0.5 * bound).all()
            live = bound > 0
            if live.any():
                worst_n = max(worst_n, float((err[live] / bound[live]).max()))
        T = R.truth_interpolate(dim, S, fi, order, X, diff, lists=lists, r=r)
        got = R.replay_interpolate(dim, S, fi, order, X, diff, lists=lists, r=r)
        bound = R.continuous_bound(dim, S, fi, order, X, diff, lists, r)
        assert np.array_equal(np.isnan(T), g["empty"]) and np.array_equal(np.isnan(got), g["empty"])
        if diff >= g["max_no"]:
            assert (T[~g["empty"]] == 0).all() and (got[~g["empty"]] == 0.0).all()
        ok = ~g["empty"]
        err = np.abs((got[ok] - T[ok]).astype(np.float64))
        assert (err <= 0.5 * bound[ok]).all(), (diff, float((err / bound[ok]).max()))
        live = bound[ok] > 0
        if live.any():
            worst_c = max(worst_c, float((err[live] / bound[ok][live]).max()))
    print("dim %d: largest fp64 replay error / bound: nearest %.3f, continuous %.3f (each must stay under 0.5)" % (dim, worst_n, worst_c))
