#!/usr/bin/env python
"""Interpolation plans against the per-call route, ALTERNATED in one process on one GPU (the boxes of a pool differ by several per
cent: a ratio is only good inside one process):
    python tools/time_interp_plan.py [--n 1000000] [--alternations 7] [--workloads 2D,3D] [--out profiles/interp_plan_timings.json]
Workloads: the C2 cloud (2D order 2, n models) evaluated on a 1024 x 1024 grid, and the C5 cloud (3D order 2) on a 128^3 grid; both
modes, the continuous radius chosen for about 12 models per point.  Routes, per mode, every one of them producing all `no` diffs:
  (a) ExpertSolver.interpolate() from host arrays, once per diff (the existing route: upload, search, evaluate, download) — wall clock;
  (b) plan.evaluate(d), one launch per diff — HIP events around the `no` launches;
  (c) plan.evaluate(range(no)), one launch — HIP events;
and the time to build the plan (wall clock around the constructor and a synchronise).  Reported: medians of `alternations` rounds after a
warm-up of every route, (c)'s algorithmic bytes per point (the point, the index or the list, the gathered origins, orders and coefficient
rows, 8 ndiff bytes out) as a fraction of the 8 TB/s HBM peak, the ratios (a)/(c) and (b)/(c), and the spread (max - min) / median of (c)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "python-wlsqm_amd"))
import torch  # noqa: E402
import bench  # noqa: E402
import wlsqm  # noqa: E402

WORKLOADS = {"2D": "C2", "3D": "C5"}


REPS = 20                           # back-to-back repetitions between the two events of one timing of (b) or (c)


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS


def wall(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--workloads", default="2D,3D")
    ap.add_argument("--grid2", type=int, default=1024, help="side of the 2D evaluation grid")
    ap.add_argument("--grid3", type=int, default=128, help="side of the 3D evaluation grid")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.alternations >= 5, "at least 5 alternations"
    dev = torch.device("cuda", 0)
    record = {"device": torch.cuda.get_device_name(0), "nmodels": a.n, "alternations": a.alternations, "hbm_peak_GBps": bench.HBM_PEAK_GBPS,
              "method": "routes alternated in one process; (a) wall clock, (b) and (c) HIP events; medians", "workloads": {}}
    for name in a.workloads.split(","):
        cfg = bench.CONFIGS[WORKLOADS[name]]
        dim, order, nk = cfg["dim"], cfg["order"], cfg["nk"]
        no = bench.NDOF[dim][order]
        S, F, hoods = bench.build_problem(cfg, a.n, 0, device=dev)
        S_d, F_d = torch.from_numpy(np.ascontiguousarray(S)).to(dev), torch.from_numpy(np.ascontiguousarray(F)).to(dev)
        h_d = torch.from_numpy(hoods.astype(np.int64)).to(dev)
        solver = wlsqm.ExpertSolver(dimension=dim, nk=np.full(a.n, nk, np.int32), order=np.full(a.n, order, np.int32),
                                    knowns=np.zeros(a.n, np.int64), weighting_method=np.full(a.n, cfg["wm"], np.int32))
        solver.prepare_device(S_d, S_d[h_d].contiguous())
        fi = torch.zeros((a.n, no), dtype=torch.float64, device=dev)
        solver.solve_device(F_d[h_d].contiguous(), fi)
        del h_d
        solver.prep_interpolate()
        side = a.grid2 if dim == 2 else a.grid3
        axes = [np.linspace(0.0, 1.0, side)] * dim
        X = np.ascontiguousarray(np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, dim))
        X_d = torch.from_numpy(X).to(dev)
        nx = X.shape[0]
        r = float(np.sqrt(12.0 / (np.pi * a.n))) if dim == 2 else float((12.0 / (4.0 / 3.0 * np.pi * a.n)) ** (1.0 / 3.0))
        diffs = list(range(no))
        rec = {"dimension": dim, "order": order, "no": no, "nx": nx, "grid_side": side, "r_continuous": r, "modes": {}}
        for mode in ("nearest", "continuous"):
            rr = r if mode == "continuous" else None
            build, plan = [], None
            for _ in range(3):
                if plan is not None:
                    plan.close()
                torch.cuda.synchronize(); t0 = time.perf_counter()
                plan = solver.interpolation_plan(X_d, mode=mode, r=rr)
                torch.cuda.synchronize(); build.append((time.perf_counter() - t0) * 1e3)
            out = torch.empty((no, nx), dtype=torch.float64, device=dev)
            one = torch.empty((nx,), dtype=torch.float64, device=dev)
            host = {}

            def route_a():
                for d in diffs:
                    host[d] = solver.interpolate(X, mode=mode, r=rr, diff=d)[0]

            def route_b():
                for d in diffs:
                    plan.evaluate(d, out=one)

            def route_c():
                plan.evaluate(diffs, out=out)

            route_a(); route_b(); route_c(); route_c()                # warm-up of every route
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            ref = np.stack([host[d] for d in diffs])
            nan_differs = int((np.isnan(got) != np.isnan(ref)).sum())  # (an origin within rounding of the sphere may fall either way)
            ok = ~np.isnan(ref) & ~np.isnan(got)
            rel = float(np.abs(got[ok] - ref[ok]).max() / max(np.abs(ref[ok]).max(), 1.0))
            for d in diffs:                                           # (b) and (c) are the same bits
                plan.evaluate(d, out=one)
                assert torch.equal(one.view(torch.int64), out[d].view(torch.int64)), d
            ms = {"a": [], "b": [], "c": []}
            for _ in range(a.alternations):
                ms["a"].append(wall(route_a)); ms["b"].append(events(route_b)); ms["c"].append(events(route_c))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            if mode == "nearest":
                mean_len = 1.0
                bytes_pt = 8 * dim + 8 + (8 * dim + 4 + 8 * no) + 8 * no
            else:
                off, _ = plan.lists()
                mean_len = float(off[-1]) / nx
                bytes_pt = 8 * dim + 8 + mean_len * (4 + 8 * dim + 4 + 8 * no) + 8 * no
            m = {"plan_build_ms": float(np.median(build)), "plan_bytes": plan.memory_used(), "mean_list_length": mean_len,
                 "a_host_interpolate_per_diff_ms": med["a"], "b_plan_one_launch_per_diff_ms": med["b"], "c_plan_all_diffs_one_launch_ms": med["c"],
                 "ms_all": {k: [round(v, 5) for v in ms[k]] for k in ms},
                 "ratio_a_over_c": med["a"] / med["c"], "ratio_b_over_c": med["b"] / med["c"],
                 "c_spread": (max(ms["c"]) - min(ms["c"])) / med["c"],
                 "c_algorithmic_bytes_per_point": bytes_pt,
                 "c_hbm_frac": bytes_pt * nx / (med["c"] * 1e-3) / (bench.HBM_PEAK_GBPS * 1e9),
                 "largest_difference_c_against_a_relative": rel, "values_where_only_one_route_is_nan": nan_differs,
                 "reps_per_timing_b_c": REPS}
            rec["modes"][mode] = m
            print("%s %-10s build %.2f ms | (a) %.2f ms  (b) %.4f ms  (c) %.4f ms | a/c %.0f  b/c %.2f | (c): %.0f B/point, %.3f of peak, "
                  "spread %.1f %% | c vs a %.1e" % (name, mode, m["plan_build_ms"], med["a"], med["b"], med["c"], m["ratio_a_over_c"],
                                                   m["ratio_b_over_c"], bytes_pt, m["c_hbm_frac"], 100 * m["c_spread"], rel), flush=True)
            plan.close()
        record["workloads"][name] = rec
        solver.close()
        del S_d, F_d, fi, X_d
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
