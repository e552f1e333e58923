#!/usr/bin/env python
"""The adjoint of interpolation plans, its routes ALTERNATED in one process on one GPU (the boxes of a pool differ by several per cent: a
ratio is only good inside one process):
    python tools/time_interp_plan_adjoint.py [--n 1000000] [--alternations 7] [--workloads 2D,3D] [--out profiles/interp_plan_adjoint_timings.json]
Workloads: the C2 cloud (2D order 2, n models) with a 1024 x 1024 grid of points, and the C5 cloud (3D order 2) with a 128^3 grid; both
modes, the continuous radius chosen for about 12 models per point; all `no` diffs, one field.  Timed, per mode:
  (a) plan.evaluate_adjoint(g, range(no)) with the inverted index present — HIP events;
  (b) today's route, nearest mode only: the scaled monomials by torch operations and one index_add_ (float atomics) — HIP events;
  (c) the forward plan.evaluate(range(no)) of the same plan — HIP events;
  (d) plan.prepare_adjoint() on a fresh plan (the sort and the offsets; it synchronises) — wall clock;
  (e) nearest mode only: (a) on a SKEWED plan whose I sends 10 % of the points to 100 models (the wave form's case).
Reported: medians of `alternations` rounds after a warm-up of every route, the spread (max - min) / median of (a), the ratios (b)/(a) and
(a)/(c), and (a)'s algorithmic bytes per point by the traffic model of DESIGN.md section 14 as a fraction of the 8 TB/s HBM peak:
    per entry   4 (tpt) + 8 dim (x_m, gathered) + 8 no (g, gathered) [+ 8 (W_m), continuous]
    per model   16 (toff pair) + 8 dim (xi) + 4 (order) + 8 no (the row, written)
divided by the number of points."""
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
import wlsqm.hip as whip  # noqa: E402

WORKLOADS = {"2D": "C2", "3D": "C5"}
REPS = 20                           # back-to-back repetitions between the two events of one timing
# exponents of the DOFs up to order 2 (wlsqm.fitter.defs)
EXPONENTS = {2: [(0, 0, 0), (1, 0, 0), (0, 1, 0), (2, 0, 0), (1, 1, 0), (0, 2, 0)],
             3: [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 0, 0), (1, 1, 0), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 1)]}
FACT = (1.0, 1.0, 2.0)


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS


def torch_route(dim, no, xi_d, X_d, I, g, grad):
    """grad[i, a] += sum_j g[j, m] c_m[index(P_a - P_j)] over the points m of model i, by torch operations and index_add_."""
    E = EXPONENTS[dim]
    index = {e: b for b, e in enumerate(E)}
    dx = X_d - xi_d[I]
    c = []
    for e in E:
        v = torch.ones_like(dx[:, 0])
        for m in range(dim):
            if e[m]:
                v = v * dx[:, m] ** e[m] / FACT[e[m]]
        c.append(v)
    rows = []
    for a in range(no):
        acc = torch.zeros_like(dx[:, 0])
        for j in range(no):
            e = tuple(E[a][m] - E[j][m] for m in range(3))
            if min(e) >= 0:
                acc = acc + g[j] * c[index[e]]
        rows.append(acc)
    grad.zero_()
    grad.index_add_(0, I, torch.stack(rows, dim=1))
    return grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--workloads", default="2D,3D")
    ap.add_argument("--grid2", type=int, default=1024, help="side of the 2D grid of points")
    ap.add_argument("--grid3", type=int, default=128, help="side of the 3D grid of points")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.alternations >= 5, "at least 5 alternations"
    dev = torch.device("cuda", 0)
    record = {"device": torch.cuda.get_device_name(0), "nmodels": a.n, "alternations": a.alternations, "hbm_peak_GBps": bench.HBM_PEAK_GBPS,
              "method": "routes alternated in one process; (a), (b), (c), (e) HIP events around %d calls, (d) wall clock; medians" % REPS,
              "workloads": {}}
    for name in a.workloads.split(","):
        cfg = bench.CONFIGS[WORKLOADS[name]]
        dim, order = cfg["dim"], cfg["order"]
        no = bench.NDOF[dim][order]
        S, _, _ = bench.build_problem(cfg, a.n, 0, device=dev)
        xi_d = torch.from_numpy(np.ascontiguousarray(S)).to(dev)
        side = a.grid2 if dim == 2 else a.grid3
        axes = [np.linspace(0.0, 1.0, side)] * dim
        X_d = torch.from_numpy(np.ascontiguousarray(np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, dim))).to(dev)
        nx = int(X_d.shape[0])
        r = float(np.sqrt(12.0 / (np.pi * a.n))) if dim == 2 else float((12.0 / (4.0 / 3.0 * np.pi * a.n)) ** (1.0 / 3.0))
        diffs = list(range(no))
        gen = torch.Generator(device=dev).manual_seed(1)
        g = torch.randn((no, nx), dtype=torch.float64, device=dev, generator=gen)
        fi = torch.randn((a.n, no), dtype=torch.float64, device=dev, generator=gen)
        out = torch.empty((no, nx), dtype=torch.float64, device=dev)
        grad = torch.empty((a.n, no), dtype=torch.float64, device=dev)
        grad_b = torch.empty((a.n, no), dtype=torch.float64, device=dev)
        rec = {"dimension": dim, "order": order, "no": no, "nx": nx, "grid_side": side, "r_continuous": r, "modes": {}}
        for mode in ("nearest", "continuous"):
            rr = r if mode == "continuous" else None
            prepare, plan = [], None
            for _ in range(3):
                if plan is not None:
                    plan.close()
                plan = whip.InterpolationPlan(xi_d, order, X_d, mode=mode, r=rr)
                torch.cuda.synchronize(); t0 = time.perf_counter()
                assert plan.prepare_adjoint()
                torch.cuda.synchronize(); prepare.append((time.perf_counter() - t0) * 1e3)
            info = plan.adjoint_info()
            routes = {"a": lambda: plan.evaluate_adjoint(g, diffs, grad_fi=grad), "c": lambda: plan.evaluate(diffs, fi=fi, out=out)}
            if mode == "nearest":
                I = plan.I
                routes["b"] = lambda: torch_route(dim, no, xi_d, X_d, I, g, grad_b)
                gen_i = np.random.default_rng(2)
                I_skew = I.cpu().numpy().copy()
                hit = gen_i.permutation(nx)[:nx // 10]
                I_skew[hit] = gen_i.permutation(a.n)[:100][gen_i.integers(0, 100, size=len(hit))]
                skew = whip.InterpolationPlan(xi_d, order, X_d, I=torch.from_numpy(I_skew).to(dev))
                skew.prepare_adjoint()
                routes["e"] = lambda: skew.evaluate_adjoint(g, diffs, grad_fi=grad)
            for fn in routes.values():                                # warm-up of every route
                fn()
            torch.cuda.synchronize()
            kernel = None
            if mode == "nearest":                                     # (a) and (b) compute the same thing
                routes["b"](); routes["a"]()
                kernel = whip.last_kernel()
                rel = float((grad - grad_b).abs().max() / grad_b.abs().max())
                first = grad.clone()
                routes["a"]()
                assert torch.equal(first.view(torch.int64), grad.view(torch.int64))
            ms = {k: [] for k in routes}
            for _ in range(a.alternations):
                for k, fn in routes.items():
                    ms[k].append(events(fn))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            nent = info["nentries"]
            bytes_pt = (nent * (4 + 8 * dim + 8 * no + (8 if mode == "continuous" else 0)) + a.n * (16 + 8 * dim + 4 + 8 * no)) / nx
            m = {"prepare_adjoint_ms": float(np.median(prepare)), "plan_bytes": plan.memory_used(), "index": info,
                 "entries_per_model": nent / a.n, "a_evaluate_adjoint_ms": med["a"], "c_forward_evaluate_ms": med["c"],
                 "ms_all": {k: [round(v, 5) for v in ms[k]] for k in ms}, "ratio_a_over_c": med["a"] / med["c"],
                 "a_spread": (max(ms["a"]) - min(ms["a"])) / med["a"], "a_algorithmic_bytes_per_point": bytes_pt,
                 "a_hbm_frac": bytes_pt * nx / (med["a"] * 1e-3) / (bench.HBM_PEAK_GBPS * 1e9), "reps_per_timing": REPS}
            line = "%s %-10s prepare %.2f ms | (a) %.4f ms  (c) %.4f ms  a/c %.2f | (a): %.0f B/point, %.3f of peak, spread %.1f %%, %.2f entries/model, longest %d" % (
                name, mode, m["prepare_adjoint_ms"], med["a"], med["c"], m["ratio_a_over_c"], bytes_pt, m["a_hbm_frac"], 100 * m["a_spread"],
                m["entries_per_model"], info["max_len"])
            if mode == "nearest":
                sinfo = skew.adjoint_info()
                m.update({"b_torch_index_add_ms": med["b"], "ratio_b_over_a": med["b"] / med["a"], "largest_difference_a_against_b_relative": rel,
                          "kernel": kernel, "e_skewed_evaluate_adjoint_ms": med["e"], "e_index": sinfo, "ratio_e_over_a": med["e"] / med["a"]})
                line += " | (b) %.4f ms  b/a %.2f  a vs b %.1e | (e) skewed %.4f ms, %d long models, longest %d" % (
                    med["b"], m["ratio_b_over_a"], rel, med["e"], sinfo["nlong"], sinfo["max_len"])
                skew.close()
            rec["modes"][mode] = m
            print(line, flush=True)
            plan.close()
        record["workloads"][name] = rec
        del xi_d, X_d, g, fi, out, grad, grad_b
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
