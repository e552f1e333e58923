#!/usr/bin/env python
"""The adjoint of the fit against the other routes to the same numbers, ALTERNATED in one process on one GPU (the boxes of a pool differ
by several per cent: a ratio is only good inside one process):
    python tools/time_adjoint.py [--configs C2,C3,C5,C1] [--alternations 7] [--out profiles/adjoint_timings.json]
Shapes: the bench's C2 / C3 / C5 at 1M cases and C1 at 10 000 (override: --n).  Routes, HIP events around REPS back-to-back calls:
  rows     fit_many_adjoint_device, WLSQM_HIP_ADJOINT_FORM=r (a wave's 64 rows through LDS);
  lane     the same, =l (one lane per case, rows from global memory);
  default  the same with the switch unset (what a caller gets);
  forward  fit_many_device, the basic fit of the same batch;
  sens     the only route to grad_fk without the adjoint: fit_many_device with the full sensitivities (n, K, no), then
           torch.einsum("jka,ja->jk") over them.
Reported: medians of `alternations` rounds after a warm-up of every route, the bytes per case of the traffic model (xk read, g read,
grad_fk and grad_fi written) and the fraction of the 8 TB/s HBM peak that the default form's median makes of it, the ratio sens / default,
and the largest per-case distance between the rows and lane forms' grad_fk and the sens route's, relative to the case's scale."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "python-wlsqm_amd"))
import torch  # noqa: E402
import bench  # noqa: E402
import wlsqm.hip as hip  # noqa: E402

SIZES = {"C1": 10_000, "C2": 1_000_000, "C3": 1_000_000, "C5": 1_000_000}
SWITCH = "WLSQM_HIP_ADJOINT_FORM"


def events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3,C5,C1")
    ap.add_argument("--n", type=int, default=0, help="cases of every config (default: the bench's sizes)")
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.alternations >= 5, "at least 5 alternations"
    dev = torch.device("cuda", 0)
    record = {"device": torch.cuda.get_device_name(0), "alternations": a.alternations, "reps_per_timing": a.reps,
              "hbm_peak_GBps": bench.HBM_PEAK_GBPS, "method": "routes alternated in one process; HIP events; medians", "configs": {}}
    for name in a.configs.split(","):
        cfg = bench.CONFIGS[name]
        dim, order, K = cfg["dim"], cfg["order"], cfg["nk"]
        n = a.n or SIZES[name]
        no = bench.NDOF[dim][order]
        S, F, hoods = bench.build_problem(cfg, n, 0, device=dev)
        S_d, F_d = torch.from_numpy(np.ascontiguousarray(S)).to(dev), torch.from_numpy(np.ascontiguousarray(F)).to(dev)
        h_d = torch.from_numpy(np.asarray(hoods)[:n].astype(np.int64)).to(dev)
        xk, fk = S_d[h_d].contiguous(), F_d[h_d].contiguous()
        xi = S_d[:n].contiguous()
        del h_d
        nk = torch.full((n,), K, dtype=torch.int32, device=dev)
        knowns = torch.full((n,), cfg["knowns"], dtype=torch.int64, device=dev)
        wm = torch.full((n,), cfg["wm"], dtype=torch.int32, device=dev)
        g = torch.from_numpy(np.random.default_rng(0).uniform(-1.0, 1.0, (n, no))).to(dev)
        fi = torch.zeros((n, no), dtype=torch.float64, device=dev)
        fi[:, 0] = F_d[:n]
        gfk, gfi = torch.empty((n, K), dtype=torch.float64, device=dev), torch.empty((n, no), dtype=torch.float64, device=dev)
        sens = torch.empty((n, K, no), dtype=torch.float64, device=dev)
        kernels, last = {}, {}

        def adjoint(form):
            def run():
                if form is None:
                    os.environ.pop(SWITCH, None)
                else:
                    os.environ[SWITCH] = form
                hip.fit_many_adjoint_device(dim, order, xk, nk, xi, knowns, wm, g, grad_fk=gfk, grad_fi=gfi)
                kernels["default" if form is None else form] = hip.last_kernel()
                os.environ.pop(SWITCH, None)
            return run

        def forward():
            hip.fit_many_device(dim, order, xk, fk, nk, xi, fi, knowns, wm)

        def sens_route():
            hip.fit_many_device(dim, order, xk, fk, nk, xi, fi, knowns, wm, sens=sens)
            # (the columns of known DOFs hold NaN: they take no part in the contraction)
            last["grad_fk"] = torch.einsum("jka,ja->jk", torch.nan_to_num(sens) if cfg["knowns"] else sens, g)

        routes = {"rows": adjoint("r"), "lane": adjoint("l"), "default": adjoint(None), "forward": forward, "sens": sens_route}
        for fn in routes.values():                                    # warm-up of every route
            fn()
        torch.cuda.synchronize()
        # the three routes give the same numbers: per case, relative to the case's scale max_k sum_a |sens g|
        scale = torch.einsum("jka,ja->jk", torch.nan_to_num(sens).abs(), g.abs()).amax(dim=1).clamp_min(1e-300)
        agree = {}
        for form in ("r", "l"):
            adjoint(form)()
            agree[form] = float(((gfk - last["grad_fk"]).abs().amax(dim=1) / scale).max())
        del scale
        ms = {k: [] for k in routes}
        for _ in range(a.alternations):
            for k, fn in routes.items():
                ms[k].append(events(fn, a.reps))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        bytes_case = 8 * K * dim + 8 * no + 8 * K + 8 * no
        rec = {"dimension": dim, "order": order, "nk": K, "no": no, "ncases": n, "knowns": cfg["knowns"],
               "kernels": kernels, "median_ms": med, "ms_all": {k: [round(v, 5) for v in ms[k]] for k in ms},
               "spread_default": (max(ms["default"]) - min(ms["default"])) / med["default"],
               "traffic_model_bytes_per_case": bytes_case,
               "hbm_frac": {k: bytes_case * n / (med[k] * 1e-3) / (bench.HBM_PEAK_GBPS * 1e9) for k in ("rows", "lane", "default")},
               "ratio_sens_over_default": med["sens"] / med["default"], "ratio_default_over_forward": med["default"] / med["forward"],
               "largest_distance_to_sens_route_per_case": {"rows": agree["r"], "lane": agree["l"]}}
        record["configs"][name] = rec
        print("%s n=%d | rows %.4f ms  lane %.4f ms  default %.4f ms (%s)  forward %.4f ms  sens+einsum %.4f ms | %d B/case, default %.3f of peak | "
              "sens/default %.1f | vs sens route: rows %.1e lane %.1e"
              % (name, n, med["rows"], med["lane"], med["default"], kernels.get("default"), med["forward"], med["sens"], bytes_case,
                 rec["hbm_frac"]["default"], rec["ratio_sens_over_default"], agree["r"], agree["l"]), flush=True)
        del xk, fk, xi, g, fi, gfk, gfi, sens, last, S_d, F_d
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
