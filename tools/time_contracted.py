#!/usr/bin/env python
"""Accurate (mode 2) against contracted (mode 3) kernel times, ALTERNATED in one process on one GPU (the boxes of a pool differ by several
per cent: a ratio is only good inside one process):
    python tools/time_contracted.py [--n 1000000] [--alternations 7] [--reps 20] [--cases C2,C5,C2_Fknown,C2_unsorted] [--out FILE.json]
Per case: `alternations` rounds of (mode 2, mode 3), each a wlsqm.hip.time_fit_device of `reps` back-to-back launches between HIP events,
after a warm-up of both modes.  Reported: the median ms of each mode, the fraction of the 8 TB/s HBM peak on the algorithmic bytes
(bench.bytes_per_fit), the ratio mode 3 / mode 2 of the medians, and the spread (max - min) / median of the mode-2 repetitions — a
ratio inside that spread says nothing.  The outputs of the two modes are compared once per case (they must differ in bits: otherwise
the mode did not take)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "python-wlsqm_amd"))
import torch  # noqa: E402
import bench  # noqa: E402
import wlsqm.hip as whip  # noqa: E402

CASES = {  # name: (config of bench.py, knowns, neighbours shuffled)
    "C2": ("C2", 0, False),
    "C5": ("C5", 0, False),
    "C2_Fknown": ("C2", 1, False),
    "C2_unsorted": ("C2", 0, True),
}
KERNEL = {2: "accurate", 3: "accurate-fma"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cases", default="C2,C5,C2_Fknown,C2_unsorted")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.alternations >= 5, "at least 5 alternations"
    dev = torch.device("cuda", 0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    record = {"device": torch.cuda.get_device_name(0), "ncases": a.n, "alternations": a.alternations, "reps_per_timing": a.reps,
              "hbm_peak_GBps": bench.HBM_PEAK_GBPS, "method": "wlsqm.hip.time_fit_device, modes 2 and 3 alternated in one process", "cases": {}}
    problems = {}
    for name in a.cases.split(","):
        cname, knowns, shuffle = CASES[name]
        cfg = bench.CONFIGS[cname]
        dim, order, nk = cfg["dim"], cfg["order"], cfg["nk"]
        if cname not in problems:
            problems[cname] = bench.build_problem(cfg, a.n, 0, device=dev)
        S, F, hoods = problems[cname]
        if shuffle:
            hoods = np.random.default_rng(5).permuted(hoods, axis=1)
        S_d, F_d, h_d = t(S), t(F), t(hoods.astype(np.int64))
        xk = S_d[h_d].contiguous(); fk = F_d[h_d].contiguous(); xi = S_d.clone()
        del h_d
        no = bench.NDOF[dim][order]
        nk_d = torch.full((a.n,), nk, dtype=torch.int32, device=dev)
        wm_d = torch.full((a.n,), cfg["wm"], dtype=torch.int32, device=dev)
        kn_d = torch.full((a.n,), knowns, dtype=torch.int64, device=dev)
        fi = torch.zeros((a.n, no), dtype=torch.float64, device=dev); fi[:, 0] = F_d
        args = (dim, order, xk, fk, nk_d, xi, fi, kn_d, wm_d)
        out = {}
        for mode in (2, 3):                                        # warm-up of both modes; their outputs, once
            with whip.strict(mode):
                whip.fit_many_device(*args); whip.fit_many_device(*args)
                torch.cuda.synchronize()
                assert whip.last_kernel() == KERNEL[mode], whip.last_kernel()
            out[mode] = fi.clone()
        differ = int((out[2].view(torch.int64) != out[3].view(torch.int64)).any(dim=1).sum())
        rel = float(((out[2] - out[3]).abs().amax(dim=0) / out[2].abs().amax(dim=0).clamp_min(1e-300)).max())
        assert differ > 0, "mode 3 returned mode 2's bits"
        ms = {2: [], 3: []}
        for _ in range(a.alternations):
            for mode in (2, 3):
                with whip.strict(mode):
                    ms[mode].append(whip.time_fit_device(*args, reps=a.reps))
        B = bench.bytes_per_fit(dim, order, nk, knowns) * a.n
        med = {m: float(np.median(ms[m])) for m in ms}
        rec = {"dimension": dim, "order": order, "nk": nk, "knowns": knowns, "neighbours_sorted": not shuffle, "algorithmic_bytes": B,
               "cases_differing_in_bits": differ, "largest_relative_column_difference": rel}
        for m, key in ((2, "accurate"), (3, "contracted")):
            rec[key] = {"ms_median": med[m], "ms_min": float(min(ms[m])), "ms_max": float(max(ms[m])), "ms_all": [round(v, 5) for v in ms[m]],
                        "hbm_frac": B / (med[m] * 1e-3) / (bench.HBM_PEAK_GBPS * 1e9), "kernel": KERNEL[m]}
        rec["ratio_contracted_over_accurate"] = med[3] / med[2]
        rec["accurate_spread"] = (max(ms[2]) - min(ms[2])) / med[2]
        record["cases"][name] = rec
        print("%-12s accurate %.4f ms (frac %.3f, spread %.1f %%)   contracted %.4f ms (frac %.3f)   ratio %.3f   %d cases differ in bits, %.1e relative"
              % (name, med[2], rec["accurate"]["hbm_frac"], 100 * rec["accurate_spread"], med[3], rec["contracted"]["hbm_frac"],
                 rec["ratio_contracted_over_accurate"], differ, rel), flush=True)
        del xk, fk, xi, fi, out
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
