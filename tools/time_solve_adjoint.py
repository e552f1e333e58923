#!/usr/bin/env python
"""The adjoint of the prepared solve (ExpertSolver.solve_many_adjoint_device) on its two routes against each other and against the
forward stacked solve, ALTERNATED in one process on one GPU (the boxes of a pool differ by several per cent: a ratio is only good
inside one process; the method of tools/time_adjoint.py):
    python tools/time_solve_adjoint.py [--shapes C4:1,C4:4,...] [--alternations 7] [--out profiles/solve_adjoint_timings.json]
Shapes (1M cases each): C4 = the bench's 2D order-2 / 32-neighbour geometry with R = 1, 4, 16, 64, 256 stacked fields, C5 = 3D order 2 /
40 neighbours with R = 64, C3 = 2D order 4 / 64 neighbours with F known and R = 64.  Routes, HIP events around REPS back-to-back calls:
  operator   WLSQM_HIP_SOLVE_ADJOINT=o: the stored operator's transpose, one batched GEMM on the matrix cores (grad_fk and grad_fi);
  op_no_fi   the same with grad_fi not wanted;
  geometric  WLSQM_HIP_SOLVE_ADJOINT=g: R adjoints of the fit on the solver's resident geometry (what there was before the operator route);
  default    the switch unset (what a caller gets);
  forward    solve_many_device of the same stack, default dispatch.
Reported: medians of `alternations` rounds after a warm-up of every route (the operator is built before the clock starts), the traffic
model 8 (no + K) + 8 no KP / R bytes per case and field (+ 8 no with grad_fi) and the fraction of the 8 TB/s HBM peak it makes of the
operator route's median, next to the forward's fraction (8 (K + no) + 8 no KP / R) from the same run."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "python-wlsqm_amd"))
import torch  # noqa: E402
import bench  # noqa: E402
import wlsqm  # noqa: E402
import wlsqm.hip as hip  # noqa: E402

SWITCH = "WLSQM_HIP_SOLVE_ADJOINT"
GEOMETRY = {"C4": "C2", "C5": "C5", "C3": "C3"}                      # C4 is C2's geometry with stacked fields
DEFAULT = "C4:1,C4:4,C4:16,C4:64,C4:256,C5:64,C3:64"


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
    ap.add_argument("--shapes", default=DEFAULT)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.alternations >= 5, "at least 5 alternations"
    dev = torch.device("cuda", 0)
    record = {"device": torch.cuda.get_device_name(0), "alternations": a.alternations, "reps_per_timing": a.reps,
              "hbm_peak_GBps": bench.HBM_PEAK_GBPS, "method": "routes alternated in one process; HIP events; medians", "shapes": []}
    shapes = [(s.split(":")[0], int(s.split(":")[1])) for s in a.shapes.split(",")]
    solver, built = None, None
    for name, R in shapes:
        cfg = bench.CONFIGS[GEOMETRY[name]]
        dim, order, K = cfg["dim"], cfg["order"], cfg["nk"]
        n = a.n
        no = bench.NDOF[dim][order]
        KP = (K + 7) // 8 * 8
        if built != GEOMETRY[name]:
            if solver is not None:
                solver.close()
            S, F, hoods = bench.build_problem(cfg, n, 0, device=dev)
            S_d = torch.from_numpy(np.ascontiguousarray(S)).to(dev)
            h_d = torch.from_numpy(np.asarray(hoods)[:n].astype(np.int64)).to(dev)
            xk, xi = S_d[h_d].contiguous(), S_d[:n].contiguous()
            del h_d, S_d
            solver = wlsqm.ExpertSolver(dimension=dim, nk=np.full(n, K, np.int32), order=np.full(n, order, np.int32),
                                        knowns=np.full(n, cfg["knowns"], np.int64), weighting_method=np.full(n, cfg["wm"], np.int32))
            solver.prepare_device(xi, xk)
            assert solver.prepare_operator(), "no operator for %s" % name
            del xk, xi
            torch.cuda.empty_cache()
            built = GEOMETRY[name]
        gen = torch.Generator(device=dev).manual_seed(R)
        g = torch.rand((R, n, no), dtype=torch.float64, device=dev, generator=gen) * 2.0 - 1.0
        gfk = torch.rand((R, n, K), dtype=torch.float64, device=dev, generator=gen)       # (the forward reads it as its fk)
        gfi = torch.zeros((R, n, no), dtype=torch.float64, device=dev)
        fi = torch.zeros((R, n, no), dtype=torch.float64, device=dev)
        kernels = {}

        def adjoint(key, switch, want_fi=True):
            def run():
                if switch is None:
                    os.environ.pop(SWITCH, None)
                else:
                    os.environ[SWITCH] = switch
                solver.solve_many_adjoint_device(g, grad_fk=gfk, grad_fi=gfi if want_fi else False)
                kernels[key] = hip.last_kernel()
                os.environ.pop(SWITCH, None)
            return run

        def forward():
            solver.solve_many_device(gfk, fi)
            kernels["forward"] = hip.last_kernel()

        routes = {"operator": adjoint("operator", "o"), "op_no_fi": adjoint("op_no_fi", "o", False),
                  "geometric": adjoint("geometric", "g"), "default": adjoint("default", None), "forward": forward}
        # the two routes give the same numbers (largest per-case distance over the case's largest |grad_fk|), and a warm-up of every route
        routes["geometric"]()
        ref = gfk[0].clone()
        routes["operator"]()
        torch.cuda.synchronize()
        agree = float(((gfk[0] - ref).abs().amax(dim=1) / ref.abs().amax(dim=1).clamp_min(1e-300)).max())
        del ref
        for fn in routes.values():
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in routes}
        for _ in range(a.alternations):
            for k, fn in routes.items():
                ms[k].append(events(fn, a.reps))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        op_bytes = 8.0 * no * KP / R
        model = {"operator": 8 * (no + K) + op_bytes + 8 * no, "op_no_fi": 8 * (no + K) + op_bytes, "forward": 8 * (K + no) + op_bytes}
        frac = {k: model[k] * n * R / (med[k] * 1e-3) / (bench.HBM_PEAK_GBPS * 1e9) for k in model}
        rec = {"shape": name, "dimension": dim, "order": order, "nk": K, "no": no, "ncases": n, "knowns": cfg["knowns"], "nrhs": R,
               "kernels": kernels, "median_ms": med, "ms_per_field": {k: v / R for k, v in med.items()},
               "ms_all": {k: [round(v, 5) for v in ms[k]] for k in ms},
               "spread_operator": (max(ms["operator"]) - min(ms["operator"])) / med["operator"],
               "traffic_model_bytes_per_case_and_field": model, "hbm_frac": frac,
               "ratio_geometric_over_operator": med["geometric"] / med["operator"],
               "ratio_operator_over_forward": med["operator"] / med["forward"],
               "largest_distance_between_routes_per_case": agree}
        record["shapes"].append(rec)
        print("%s R=%d | operator %.4f ms (%.3f of peak)  no-fi %.4f (%.3f)  geometric %.4f  default %.4f (%s)  forward %.4f (%s, %.3f) | "
              "geometric / operator %.2f | routes agree to %.1e"
              % (name, R, med["operator"], frac["operator"], med["op_no_fi"], frac["op_no_fi"], med["geometric"], med["default"],
                 kernels.get("default"), med["forward"], kernels.get("forward"), frac["forward"], rec["ratio_geometric_over_operator"], agree),
              flush=True)
        del g, gfk, gfi, fi
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
