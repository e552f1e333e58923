#!/usr/bin/env python
"""The geometry adjoint of the fit against its neighbours, ALTERNATED in one process on one GPU (the boxes of a pool differ by several per
cent: a ratio is only good inside one process):
    python tools/time_geometry_adjoint.py [--configs C2,C5,C3,C1] [--alternations 7] [--out profiles/geometry_adjoint_timings.json]
Shapes: the bench's C2 / C5 / C3 at 1M cases and C1 at 4M (override: --n).  Routes, HIP events around REPS back-to-back calls:
  geometry_rows  fit_many_geometry_adjoint_device with the fused grad_fk, WLSQM_HIP_ADJOINT_FORM=r (a wave's 64 rows through LDS);
  geometry_lane  the same, =l (one lane per case, rows from global memory);
  geometry_rows_no_grad_fk  the rows form without the fused grad_fk (what the per-lane stores of grad_fk cost);
  adjoint_rows   fit_many_adjoint_device, =r: the existing adjoint, whose bytes the geometry adjoint's are apart from fk, fi and a
                 dim-times larger output;
  adjoint_lane   the same, =l;
  forward        fit_many_device, the basic fit of the same batch.
Reported: medians of `alternations` rounds after a warm-up of every route, the bytes per case of the traffic model (xk, fk, fi and g read;
grad_xk, grad_xi and grad_fk written), the fraction of the 8 TB/s HBM peak each form's median makes of it, the faster form, and the
ratios geometry_rows / adjoint_rows and faster form / forward.  The form csrc/fit_adjoint.hip runs with the switch unset
(launch_fit_geometry_adjoint) is whichever is faster in the record this writes."""
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

SIZES = {"C1": 4_000_000, "C2": 1_000_000, "C3": 1_000_000, "C5": 1_000_000}
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
    ap.add_argument("--configs", default="C2,C5,C3,C1")
    ap.add_argument("--n", type=int, default=0, help="cases of every config (default: 1M, C1 4M)")
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
        fi0 = torch.zeros((n, no), dtype=torch.float64, device=dev)
        fi0[:, 0] = F_d[:n]
        fi = fi0.clone()
        hip.fit_many_device(dim, order, xk, fk, nk, xi, fi, knowns, wm)      # fi_out of the forward fit: what the geometry adjoint reads
        fi_out = fi.clone()
        gxk, gxi = torch.empty_like(xk), torch.empty_like(xi)
        gfk, gfi = torch.empty((n, K), dtype=torch.float64, device=dev), torch.empty((n, no), dtype=torch.float64, device=dev)
        kernels = {}

        def switched(form, label, call):
            def run():
                os.environ[SWITCH] = form
                call()
                kernels[label] = hip.last_kernel()
                os.environ.pop(SWITCH, None)
            return run

        def geometry():
            hip.fit_many_geometry_adjoint_device(dim, order, xk, fk, nk, xi, fi_out, knowns, wm, g, grad_xk=gxk, grad_xi=gxi, grad_fk=gfk)

        def geometry_alone():
            hip.fit_many_geometry_adjoint_device(dim, order, xk, fk, nk, xi, fi_out, knowns, wm, g, grad_xk=gxk, grad_xi=gxi, grad_fk=False)

        def adjoint():
            hip.fit_many_adjoint_device(dim, order, xk, nk, xi, knowns, wm, g, grad_fk=gfk, grad_fi=gfi)

        def forward():
            hip.fit_many_device(dim, order, xk, fk, nk, xi, fi, knowns, wm)

        routes = {"geometry_rows": switched("r", "geometry_rows", geometry), "geometry_lane": switched("l", "geometry_lane", geometry),
                  "geometry_rows_no_grad_fk": switched("r", "geometry_rows_no_grad_fk", geometry_alone),
                  "adjoint_rows": switched("r", "adjoint_rows", adjoint), "adjoint_lane": switched("l", "adjoint_lane", adjoint),
                  "forward": forward}
        for fn in routes.values():                                    # warm-up of every route
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in routes}
        for _ in range(a.alternations):
            for k, fn in routes.items():
                ms[k].append(events(fn, a.reps))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        bytes_case = 8 * K * dim + 8 * K + 8 * no + 8 * no + 8 * K * dim + 8 * dim + 8 * K
        faster = "rows" if med["geometry_rows"] <= med["geometry_lane"] else "lane"
        rec = {"dimension": dim, "order": order, "nk": K, "no": no, "ncases": n, "knowns": cfg["knowns"],
               "kernels": kernels, "median_ms": med, "ms_all": {k: [round(v, 5) for v in ms[k]] for k in ms},
               "traffic_model_bytes_per_case": bytes_case,
               "hbm_frac": {k: bytes_case * n / (med[k] * 1e-3) / (bench.HBM_PEAK_GBPS * 1e9) for k in ("geometry_rows", "geometry_lane")},
               "faster_form": faster,
               "ratio_geometry_rows_over_adjoint_rows": med["geometry_rows"] / med["adjoint_rows"],
               "ratio_faster_over_forward": med["geometry_" + faster] / med["forward"]}
        record["configs"][name] = rec
        print("%s n=%d | geometry rows %.4f ms  lane %.4f ms (faster: %s) | adjoint rows %.4f ms  lane %.4f ms | forward %.4f ms | %d B/case, "
              "rows %.3f lane %.3f of peak | geometry rows / adjoint rows %.2f | rows without grad_fk %.4f ms"
              % (name, n, med["geometry_rows"], med["geometry_lane"], faster, med["adjoint_rows"], med["adjoint_lane"], med["forward"],
                 bytes_case, rec["hbm_frac"]["geometry_rows"], rec["hbm_frac"]["geometry_lane"],
                 rec["ratio_geometry_rows_over_adjoint_rows"], med["geometry_rows_no_grad_fk"]), flush=True)
        del xk, fk, xi, g, fi, fi0, fi_out, gxk, gxi, gfk, gfi, S_d, F_d
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
