#!/usr/bin/env python
"""The overlapping blocks of wlsqm.hip.StencilSolver (OverlappingBlocks) against "jacobi" and BlockJacobi(16) of the
same process and commit, the routes ALTERNATED on one GPU (the method of tools/time_krylov.py):
    python tools/time_krylov_schwarz.py [--shapes 2-2-24,3-2-40,2-4-64] [--n 1000000] [--alternations 7] [--maxiter 4000]
                                        [--block 32] [--rows 64] [--out profiles/krylov_schwarz_timings.json]
Clouds: those of tools/time_krylov.py (n Halton points in Morton order, K nearest neighbours, b_F known, centre weighting).
Routes: method x preconditioner, each its own solver on the one operator; HIP events around one enqueue; medians of `alternations`
rounds after a warm-up of every route.
  a. per iteration, every cloud: (I - 0.25 h^2 Lap_h) x = b with rtol = atol = 0, N = 10 and N = 20 iterations, refresh=False (the
     build is timed on its own); ms per iteration (bicgstab) or per cycle (bicgstab2) as the difference of the two runs.  The traffic
     model per point and iteration, overlapping blocks over Jacobi: two applications of 8 rows + 4 rows / block bytes of plane and table
     each, with 16 bytes of vectors, on top of the gathered vector (which the model leaves to the caches, as it does the product's):
     (24 (K + 1) + 208 + 2 (8 rows + 4 rows / block) + 16) / (24 (K + 1) + 208) (section 28 allows measured / model <= 1.15).
  b. the build: ms of solver.refresh() ("krylov-schwarz-build") against BlockJacobi(16)'s ("krylov-blocks") and one Jacobi iteration;
     the constructor's set search (torch operations, once per solver) in ms of wall time.
  c. to rtol 1e-10 from zero: I - h^2 Lap_h (tau 1) on every cloud and the Dirichlet Poisson problem on the 2D clouds, with both
     methods; the overlapping blocks with refresh=True (the build is in the time) and blocks of 16 beside.  One solve() finds the count
     and the status; the timed call is enqueue(b, x, count).  A route that does not converge within --maxiter is reported with its
     status, its residuals and the time of one run: a failure is a result."""
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
import synth  # noqa: E402
import wlsqm  # noqa: E402
import wlsqm.hip as hip  # noqa: E402

N1, N2 = 10, 20
BLOCK = 16
SETS = [32, 64]                      # --block, --rows
PRECONDS = ("jacobi", "block%d" % BLOCK, "schwarz")
METHODS = ("bicgstab", "bicgstab2")


def key(route):
    return "%s/%s" % route


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def preconditioner(pc, refresh):
    return pc if pc == "jacobi" else hip.BlockJacobi(BLOCK, refresh=refresh) if pc.startswith("block") else hip.OverlappingBlocks(SETS[0], SETS[1], refresh=refresh)


def per_iteration(op, b, n, K, scale, alternations):
    routes = [(method, pc) for pc in PRECONDS for method in METHODS]
    solvers = {k: hip.StencilSolver(op, diag=1.0, scale=scale, method=k[0], preconditioner=preconditioner(k[1], False)) for k in routes}
    x = torch.zeros(n, dtype=torch.float64, device=b.device)

    def run(k, N):
        x.zero_()
        return events(lambda: solvers[k].enqueue(b, x, N, rtol=0.0))

    for k in routes:
        run(k, N1); run(k, N2)
    ms = {k: {N1: [], N2: []} for k in routes}
    build = {pc: [] for pc in PRECONDS[1:]}
    early = []
    for _ in range(alternations):
        for k in routes:
            for N in (N1, N2):
                ms[k][N].append(run(k, N))
                got = solvers[k].info()
                if (got.status, got.iterations) != (1, N):
                    early.append((key(k), N, got.status, got.iterations))
        for pc in build:
            build[pc].append(events(lambda: solvers["bicgstab", pc].refresh()))
    med = {k: {N: float(np.median(v)) for N, v in ms[k].items()} for k in routes}
    per = {k: (2 if k[0] == "bicgstab2" else 1) * (med[k][N2] - med[k][N1]) / (N2 - N1) for k in routes}      # an iteration, or a cycle
    jacobi = 24 * (K + 1) + 208
    model = (jacobi + 2 * (8 * SETS[1] + 4 * SETS[1] / SETS[0]) + 16) / jacobi
    out = {"ms_per_iteration_or_cycle": {key(k): per[k] for k in routes},
           "median_ms": {key(k): {str(N): v for N, v in med[k].items()} for k in routes},
           "ms_all": {key(k): {str(N): [round(v, 5) for v in vs] for N, vs in ms[k].items()} for k in routes},
           "stopped_early": early, "solver_memory_bytes": {key(k): s.memory_used() for k, s in solvers.items()},
           "build_ms": {pc: float(np.median(v)) for pc, v in build.items()}, "build_ms_all": {pc: [round(t, 4) for t in v] for pc, v in build.items()},
           "model_ratio_schwarz_over_jacobi": model, "schwarz_over_jacobi": {}, "schwarz_over_block": {}, "over_model": {}}
    for method in METHODS:
        out["schwarz_over_jacobi"][method] = per[method, "schwarz"] / per[method, "jacobi"]
        out["schwarz_over_block"][method] = per[method, "schwarz"] / per[method, "block%d" % BLOCK]
        out["over_model"][method] = out["schwarz_over_jacobi"][method] / model
    out["build_over_jacobi_iteration"] = out["build_ms"]["schwarz"] / per["bicgstab", "jacobi"]
    out["build_over_blocks_build"] = out["build_ms"]["schwarz"] / out["build_ms"]["block%d" % BLOCK]
    for s in solvers.values():
        s.close()
    return out


def to_tolerance(op, b, n, diag, scale, alternations, maxiter):
    routes = [(method, pc) for pc in ("schwarz", "block%d" % BLOCK) for method in METHODS]
    solvers = {k: hip.StencilSolver(op, diag=diag, scale=scale, method=k[0], preconditioner=preconditioner(k[1], True)) for k in routes}
    x = torch.zeros(n, dtype=torch.float64, device=b.device)
    res = torch.empty(n, dtype=torch.float64, device=b.device)
    found = {}
    for k in routes:                                                     # the count and the status; also the warm-up
        x.zero_()
        info = solvers[k].solve(b, x, rtol=1e-10, maxiter=maxiter, check_every=64)
        solvers[k].product(x, out=res)
        found[k] = {"status": info.status, "iterations": info.iterations, "recursive_residual_over_b": info.residual / float(b.norm()),
                    "true_residual_over_b": float((b - res).norm() / b.norm())}
    ms = {k: [] for k in routes}
    for it in range(alternations):
        for k in routes:
            if found[k]["status"] != 0 and it > 0:                       # a run to the iteration limit is timed once
                continue
            x.zero_()
            N = max(found[k]["iterations"], 1) if found[k]["status"] == 0 else maxiter
            ms[k].append(events(lambda: solvers[k].enqueue(b, x, N, rtol=1e-10)))
            got = solvers[k].info()
            assert got.iterations == found[k]["iterations"], (k, got, found[k])
    for s in solvers.values():
        s.close()
    for k in routes:
        found[k]["total_ms"] = float(np.median(ms[k]))
        found[k]["ms_all"] = [round(v, 4) for v in ms[k]]
    return {key(k): v for k, v in found.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2-2-24,3-2-40,2-4-64", help="dimension-order-neighbours, comma separated")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--maxiter", type=int, default=4000)
    ap.add_argument("--block", type=int, default=32)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    SETS[:] = [a.block, a.rows]
    assert a.alternations >= 5, "at least 5 alternations"
    dev = torch.device("cuda", 0)
    record = {"device": torch.cuda.get_device_name(0), "alternations": a.alternations, "npoints": a.n, "iterations": [N1, N2],
              "maxiter": a.maxiter, "block": a.block, "rows": a.rows, "hbm_peak_GBps": bench.HBM_PEAK_GBPS,
              "method": "routes alternated in one process; HIP events around one enqueue; medians; ms per iteration (bicgstab) or cycle "
                        "(bicgstab2) from the difference of 20 and 10 iterations with refresh=False; build_ms = solver.refresh(); total_ms = "
                        "enqueue of the count that solve() found (of maxiter, once, where it did not converge), refresh=True, to rtol 1e-10 "
                        "from zero, stopping on the device",
              "shapes": {}}
    for shape in a.shapes.split(","):
        dim, order, K = (int(v) for v in shape.split("-"))
        n = a.n
        S = torch.from_numpy(synth.halton(n, dim)).to(dev)
        S = S[bench.morton_order_device(S)].contiguous()
        hoods = hip.knn(S, K)
        nk = torch.full((n,), K, dtype=torch.int32, device=dev)
        knowns = torch.full((n,), 1, dtype=torch.int64, device=dev)
        wm = torch.full((n,), wlsqm.WEIGHT_CENTER, dtype=torch.int32, device=dev)
        lap = hip.stencil_rows(dim, order, "laplacian", device=dev)
        op = hip.StencilOperator(dim, order, S, hoods, nk, knowns, wm, lap)
        h2 = n ** (-2.0 / dim)
        b = torch.sin(3 * S[:, 0]) * torch.cos(2 * S[:, -1])
        rec = {"dimension": dim, "order": order, "nk": K, "npoints": n, "fill": op.fill, "stored_entries": op._m["total"],
               "per_iteration": per_iteration(op, b, n, K, -0.25 * h2, a.alternations), "to_rtol_1e-10": {}}
        p = rec["per_iteration"]
        print("%s n=%d | ms per iteration / cycle %s | overlapping blocks over jacobi %s, the model's %.3f, over the model %s | build ms %s (%.1f Jacobi "
              "iterations, %.1f krylov-blocks)"
              % (shape, n, " ".join("%s %.4f" % kv for kv in p["ms_per_iteration_or_cycle"].items()),
                 " ".join("%s %.3f" % kv for kv in p["schwarz_over_jacobi"].items()), p["model_ratio_schwarz_over_jacobi"],
                 " ".join("%.3f" % v for v in p["over_model"].values()), " ".join("%s %.3f" % kv for kv in p["build_ms"].items()),
                 p["build_over_jacobi_iteration"], p["build_over_blocks_build"]), flush=True)
        if p["stopped_early"]:
            print("  NOT VALID: solves stopped before their iteration limit: %s" % p["stopped_early"][:4], flush=True)
        t0 = time.perf_counter()
        hip.overlapping_sets(op._m, a.block, a.rows)
        torch.cuda.synchronize()
        rec["set_search_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        print("  the set search: %.1f ms of wall time" % rec["set_search_wall_ms"], flush=True)
        systems = [("tau1", op, 1.0, -1.0 * h2)]
        dirichlet = None
        if dim == 2:
            band = (torch.minimum(S, 1.0 - S).min(dim=1).values < 1.2 * n ** (-1.0 / dim))
            e_f = hip.stencil_rows(dim, order, "value", device=dev)
            rows = torch.where(band[:, None], e_f[0][None, :], -lap[0][None, :])[None].contiguous()
            dirichlet = hip.StencilOperator(dim, order, S, hoods, nk, knowns, wm, rows)
            systems.append(("dirichlet", dirichlet, 0.0, 1.0))
        for what, sys_op, diag, scale in systems:
            found = to_tolerance(sys_op, b, n, diag, scale, a.alternations, a.maxiter)
            rec["to_rtol_1e-10"][what] = found
            print("  %s to rtol 1e-10 | %s" % (what, " | ".join("%s %d its (status %d) %.2f ms, true %.1e"
                  % (k, v["iterations"], v["status"], v["total_ms"], v["true_residual_over_b"]) for k, v in found.items())), flush=True)
        if dirichlet is not None:
            dirichlet.close()
        record["shapes"][shape] = rec
        if a.out:                                                        # what is measured so far, shape by shape
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(record, f, indent=1)
                f.write("\n")
        op.close()
        del S, hoods, b, op, dirichlet
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
