"""The LDS-DMA form of the staged kernel for the dense 2D systems up to 6 unknowns (csrc/fit_stage.hip, PART = 6: the default for rows of
whole 128-byte lines on line-aligned bases) against the register-staged form it replaced there: the SAME bits per case, on the same device
tensors.  WLSQM_HIP_STAGE_DMA6=0 brings the register-staged kernel back; a launch whose bases are not on a line takes it by itself — both
show as "stage-reg" in wlsqm.hip.last_kernel().  Rows that are not whole lines (the values' rows: K not a multiple of 16) are the
register-staged kernel's as before ("stage", whatever the switch says).  Every case names the labels it expects, the tile kernels' included
(2D order 2 below 32 neighbours, 2D order 1), so that a change of dispatch shows here and is not taken for agreement of the two forms: the
LDS-DMA form itself runs at K = 32, 48, 64 and 80 only — the staged kernel has no row of one chunk or of one pair by the dispatch."""
import numpy as np
import pytest

import _cases as K
import _parity as P

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def wlsqm():
    import wlsqm as W
    from wlsqm import _binding
    assert _binding.lib().wlsqm_hip_device_count() >= 1, "no HIP device: the GPU tests need a real MI355X"
    return W


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _batch(W, Kn, n, order, rows, ragged, knowns, weighting, seed):
    """rows: 'sorted' (by distance, what a k-nearest-neighbour search returns), 'shuffled' (every wave repeats its pass), 'one' (sorted except
    one case per wave of 64).  ragged: nk below K for some cases, NaN in their padding slots."""
    rng = np.random.default_rng(seed)
    no = K.NDOF[2][order]
    xi = rng.uniform(0, 1, (n, 2))
    off = 0.05 * rng.uniform(-1, 1, (n, Kn, 2))
    srt = np.take_along_axis(off, np.argsort((off ** 2).sum(axis=2), axis=1, kind="stable")[..., None], axis=1)
    if rows == "sorted":
        off = srt
    elif rows == "one":
        pick = (np.arange(n) % 64) == 37 % min(n, 64)
        off = np.where(pick[:, None, None], off, srt)
    xk = xi[:, None, :] + off
    fk = np.sin(3 * xk[..., 0]) * np.cos(2 * xk[..., 1])
    nk = np.full(n, Kn, np.int32)
    if ragged:
        nk[::5] = Kn - 1; nk[3::11] = Kn - 7; nk[n // 2] = max(Kn - 9, 7)
        for j in np.nonzero(nk < Kn)[0]:
            xk[j, nk[j]:] = np.nan; fk[j, nk[j]:] = np.nan
    kn = np.full(n, knowns, np.int64)
    wm = np.full(n, weighting, np.int32)
    fi0 = rng.uniform(-1, 1, (n, no))
    fi0[:, 0] = np.sin(3 * xi[:, 0]) * np.cos(2 * xi[:, 1])
    return dict(xk=xk, fk=fk, nk=nk, xi=xi, kn=kn, wm=wm, fi0=fi0, order=order, no=no)


def _both_forms(monkeypatch, b, xk_d, fk_d, expect):
    """Runs the previous form (switch off) and the default on the same device tensors; returns the default's result (bits asserted equal)
    and the labels.  expect: the labels of (previous form, default) — where they are the same, one kernel ran twice and the comparison only
    says that the switch changes nothing there."""
    import torch
    import wlsqm.hip as whip
    rest = (_t(b["nk"]), _t(b["xi"]))
    tail = (_t(b["kn"]), _t(b["wm"]))
    out, label = {}, {}
    for sw in ("0", "1"):
        if sw == "0":
            monkeypatch.setenv("WLSQM_HIP_STAGE_DMA6", "0")
        else:
            monkeypatch.delenv("WLSQM_HIP_STAGE_DMA6")
        fi = _t(b["fi0"])
        whip.fit_many_device(2, b["order"], xk_d, fk_d, *rest, fi, *tail)
        torch.cuda.synchronize()
        out[sw], label[sw] = fi.cpu().numpy(), whip.last_kernel()
    assert (label["0"], label["1"]) == expect, (label, expect)
    assert np.array_equal(out["0"].view(np.int64), out["1"].view(np.int64)), "the two forms differ in %d of %d cases" % (
        (out["0"].view(np.int64) != out["1"].view(np.int64)).any(axis=1).sum(), len(out["0"]))
    known = np.array([[(int(k) >> a) & 1 for a in range(b["no"])] for k in b["kn"]], bool)
    assert np.array_equal(out["1"][known].view(np.int64), b["fi0"][known].view(np.int64)), "a known DOF did not come back with its own bits"
    return out["1"], label


DMA6 = ("stage-reg", "stage")        # rows of whole lines on line-aligned bases: the switch picks between the two forms
OFF_LINE = ("stage-reg", "stage-reg")  # whole lines, a base off a line: the register-staged kernel either way
OTHER_K = ("stage", "stage")           # rows that are not whole lines: as before
TILE = ("tile", "tile")                # 2D order 2 below 32 neighbours and 2D order 1: the tile kernels', not the staged kernel's

EXPECT = {8: TILE, 16: TILE, 32: DMA6, 34: OTHER_K, 40: OTHER_K, 48: DMA6, 64: DMA6, 80: DMA6}


# (K, cases, rows, ragged, knowns, weighting, also against the CPU oracle)
CASES = [
    (32, 197, "sorted", False, 0, "CENTER", True),
    (32, 65, "shuffled", False, 1, "CENTER", False),
    (32, 64, "one", True, 0b101, "UNIFORM", False),
    (32, 1, "sorted", False, 0, "CENTER", False),
    (32, 63, "sorted", True, 1, "UNIFORM", False),
    (32, 197, "one", True, 0, "CENTER", False),
    (48, 197, "shuffled", True, 0b101, "CENTER", True),      # six chunks
    (64, 65, "one", True, 1, "UNIFORM", False),               # eight chunks
    (80, 197, "sorted", True, 0, "CENTER", True),             # ten chunks: the values' rows are five lines
    (8, 65, "sorted", False, 0, "CENTER", True),              # a single chunk: the tile kernel's
    (16, 197, "sorted", True, 1, "CENTER", True),             # one pair: the tile kernel's
    (34, 197, "sorted", True, 0, "CENTER", True),             # a partial last chunk: rows are not whole lines
    (34, 64, "shuffled", False, 0b101, "UNIFORM", False),
    (40, 65, "one", True, 1, "CENTER", True),                 # an odd chunk count: the values' rows are not whole lines
    (40, 197, "sorted", False, 0, "UNIFORM", False),
]


@pytest.mark.parametrize("Kn,n,rows,ragged,knowns,weighting,check", CASES)
def test_dma_form_gives_the_previous_forms_bits(wlsqm, oracle, monkeypatch, Kn, n, rows, ragged, knowns, weighting, check):
    b = _batch(wlsqm, Kn, n, 2, rows, ragged, knowns, getattr(wlsqm, "WEIGHT_" + weighting), 1000 * Kn + n)
    got, label = _both_forms(monkeypatch, b, _t(b["xk"]), _t(b["fk"]), expect=EXPECT[Kn])
    assert not np.isnan(got).any(), "a padding slot was read"
    if check:
        oa = np.full(n, 2, np.int32)
        xk0, fk0 = np.nan_to_num(b["xk"]), np.nan_to_num(b["fk"])
        ref = b["fi0"].copy()
        oracle.fit_many(2, xk0, fk0, b["nk"], b["xi"], ref, None, 0, oa, b["kn"], b["wm"], ntasks=8)
        truth = P.truth_fit(2, xk0, fk0, b["nk"], b["xi"], b["fi0"], oa, b["kn"], b["wm"])
        P.assert_parity(got, ref, truth, "LDS-DMA form, K = %d" % Kn)


def test_order_1_runs_one_kernel_whatever_the_switch(wlsqm, monkeypatch):
    """2D order 1 (3 unknowns) is the tile kernel's at every K: the switch must change neither the kernel nor the bits."""
    b = _batch(wlsqm, 32, 197, 1, "sorted", True, 1, wlsqm.WEIGHT_CENTER, 7)
    _both_forms(monkeypatch, b, _t(b["xk"]), _t(b["fk"]), expect=TILE)


@pytest.mark.parametrize("skip_bytes", [16, 64])
def test_bases_off_a_line_take_the_previous_form(wlsqm, monkeypatch, skip_bytes):
    """xk and fk as slices that start 16 / 64 bytes into a larger allocation: not on a line, so the launch keeps the register-staged kernel."""
    import torch
    b = _batch(wlsqm, 32, 197, 2, "sorted", True, 1, wlsqm.WEIGHT_CENTER, 31 + skip_bytes)
    s = skip_bytes // 8
    xbuf = torch.zeros(s + b["xk"].size + 64, dtype=torch.float64, device="cuda:0")
    fbuf = torch.zeros(s + b["fk"].size + 64, dtype=torch.float64, device="cuda:0")
    xk_d = xbuf[s:s + b["xk"].size].view(b["xk"].shape); xk_d.copy_(_t(b["xk"]))
    fk_d = fbuf[s:s + b["fk"].size].view(b["fk"].shape); fk_d.copy_(_t(b["fk"]))
    assert xk_d.data_ptr() % 128 == skip_bytes and fk_d.data_ptr() % 128 == skip_bytes
    got, _ = _both_forms(monkeypatch, b, xk_d, fk_d, expect=OFF_LINE)
    ref, _ = _both_forms(monkeypatch, b, _t(b["xk"]), _t(b["fk"]), expect=DMA6)
    assert np.array_equal(got.view(np.int64), ref.view(np.int64))


@pytest.mark.parametrize("n", [197, 64])
def test_rows_that_end_their_allocation(wlsqm, monkeypatch, n):
    """xk and fk END with their 2 MiB tensors (and start on a line: the rows are whole lines), so the LDS-DMA form runs with nothing of the
    tensor behind the last row.  What this shows is identical bits and no NaN there, NOT the absence of an over-read: the caching allocator
    may have carved the tensor out of a larger block, so the bytes behind it can be mapped.  That no transfer leaves [base, base + n rows)
    rests on the kernel's code: a transfer's offset is (chunk, piece, clamped to the row's last piece) in a VALID row of the group (tail
    groups and idle lanes replay the group's last valid row)."""
    import torch
    b = _batch(wlsqm, 32, n, 2, "one", True, 0, wlsqm.WEIGHT_CENTER, 5 + n)
    total = (2 << 20) // 8
    xbuf = torch.full((total,), float("nan"), dtype=torch.float64, device="cuda:0")
    fbuf = torch.full((total,), float("nan"), dtype=torch.float64, device="cuda:0")
    xk_d = xbuf[total - b["xk"].size:].view(b["xk"].shape); xk_d.copy_(_t(b["xk"]))
    fk_d = fbuf[total - b["fk"].size:].view(b["fk"].shape); fk_d.copy_(_t(b["fk"]))
    assert xk_d.data_ptr() % 128 == 0 and fk_d.data_ptr() % 128 == 0
    got, _ = _both_forms(monkeypatch, b, xk_d, fk_d, expect=DMA6)
    assert not np.isnan(got).any()


def test_dma_form_captured_and_replayed(wlsqm, monkeypatch):
    import torch
    import wlsqm.hip as whip
    b = _batch(wlsqm, 32, 197, 2, "sorted", True, 1, wlsqm.WEIGHT_CENTER, 77)
    xk_d, fk_d = _t(b["xk"]), _t(b["fk"])
    want, _ = _both_forms(monkeypatch, b, xk_d, fk_d, expect=DMA6)
    fi_g = _t(b["fi0"])
    args = (2, 2, xk_d, fk_d, _t(b["nk"]), _t(b["xi"]), fi_g, _t(b["kn"]), _t(b["wm"]))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        whip.fit_many_device(*args)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            whip.fit_many_device(*args)
        assert whip.last_kernel() == "stage"
        for _ in range(2):
            fi_g.copy_(_t(b["fi0"]))
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(fi_g.cpu().numpy().view(np.int64), want.view(np.int64))
