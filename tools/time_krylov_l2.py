#!/usr/bin/env python
"""BiCGSTAB(2) of wlsqm.hip.StencilSolver (method="bicgstab2") against the BiCGSTAB of the same process and commit,
the routes ALTERNATED on one GPU (the method of tools/time_krylov.py: a ratio is only good inside one process):
    python tools/time_krylov_l2.py [--shapes 2-2-24,3-2-40,2-4-64] [--n 1000000] [--alternations 7] [--maxiter 4000]
                                   [--out profiles/krylov_l2_timings.json]
Clouds: those of tools/time_krylov.py (n Halton points in Morton order, K nearest neighbours, b_F known, centre weighting).
Routes: method x preconditioner, "bicgstab" and "bicgstab2" with "jacobi" and BlockJacobi(16), each its own solver on the one operator;
HIP events around one enqueue; medians of `alternations` rounds after a warm-up of every route.
  a. per cycle, every cloud: (I - 0.25 h^2 Lap_h) x = b with rtol = atol = 0, N = 10 and N = 20 iterations (5 and 10 cycles); ms per
     cycle against ms per TWO iterations of BiCGSTAB, each the difference of the two runs.  A timed run that does not end with status 1
     at exactly N iterations is listed under stopped_early.  The traffic model (section 21): both take 4 passes over 12 bytes per stored
     entry and 4 reads of 4 bytes per point; a cycle has 57 vector accesses of 8 bytes per point where two iterations have 50, and with
     blocks 5 streams of 8 * block bytes per point where two iterations have 4.  `over_model` is the measured ratio over the model's
     (section 21 expects <= 1.15).
  b. to rtol 1e-10 from zero: I - tau h^2 Lap_h at tau 0.25 and 1 and the Dirichlet Poisson problem (-Lap_h inside, identity rows within
     1.2 h of the boundary) on the 2D clouds, tau 1 alone on the 3D cloud.  One solve() finds the count and the status; the timed call
     is enqueue(b, x, count), which stops on the device with no host read.  A route that does not converge within --maxiter is reported
     with its status and the time of its run: a failure is a result."""
import argparse
import json
import os
import sys

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
ROUTES = [(method, pc) for pc in ("jacobi", "block%d" % BLOCK) for method in ("bicgstab", "bicgstab2")]


def key(route):
    return "%s/%s" % route


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def solvers_of(op, diag, scale):
    return {(method, pc): hip.StencilSolver(op, diag=diag, scale=scale, method=method,
                                            preconditioner="jacobi" if pc == "jacobi" else hip.BlockJacobi(BLOCK)) for method, pc in ROUTES}


def per_cycle(op, b, n, scale, alternations):
    solvers = solvers_of(op, 1.0, scale)
    x = torch.zeros(n, dtype=torch.float64, device=b.device)

    def run(k, N):
        x.zero_()
        return events(lambda: solvers[k].enqueue(b, x, N, rtol=0.0))

    for k in ROUTES:
        run(k, N1); run(k, N2)
    ms = {k: {N1: [], N2: []} for k in ROUTES}
    early = []
    for _ in range(alternations):
        for k in ROUTES:
            for N in (N1, N2):
                ms[k][N].append(run(k, N))
                got = solvers[k].info()
                if (got.status, got.iterations) != (1, N):
                    early.append((key(k), N, got.status, got.iterations))
    med = {k: {N: float(np.median(v)) for N, v in ms[k].items()} for k in ROUTES}
    per_two = {k: 2 * (med[k][N2] - med[k][N1]) / (N2 - N1) for k in ROUTES}            # a cycle, or two iterations
    total = op._m["total"]
    matrix = 4 * total * (4 + 8) + n * 4 * 4
    model = {("bicgstab", "jacobi"): matrix + n * 50 * 8, ("bicgstab2", "jacobi"): matrix + n * 57 * 8,
             ("bicgstab", "block%d" % BLOCK): matrix + n * (50 * 8 + 4 * 8 * BLOCK), ("bicgstab2", "block%d" % BLOCK): matrix + n * (57 * 8 + 5 * 8 * BLOCK)}
    out = {"ms_per_cycle_or_two_iterations": {key(k): per_two[k] for k in ROUTES},
           "median_ms": {key(k): {str(N): v for N, v in med[k].items()} for k in ROUTES},
           "ms_all": {key(k): {str(N): [round(v, 5) for v in vs] for N, vs in ms[k].items()} for k in ROUTES},
           "traffic_model_bytes": {key(k): model[k] for k in ROUTES},
           "hbm_frac": {key(k): model[k] / (per_two[k] * 1e-3) / (bench.HBM_PEAK_GBPS * 1e9) for k in ROUTES},
           "stopped_early": early, "solver_memory_bytes": {key(k): s.memory_used() for k, s in solvers.items()},
           "cycle_over_two_iterations": {}, "model_ratio": {}, "over_model": {}}
    for pc in ("jacobi", "block%d" % BLOCK):
        ratio, model_ratio = per_two["bicgstab2", pc] / per_two["bicgstab", pc], model["bicgstab2", pc] / model["bicgstab", pc]
        out["cycle_over_two_iterations"][pc], out["model_ratio"][pc], out["over_model"][pc] = ratio, model_ratio, ratio / model_ratio
    for s in solvers.values():
        s.close()
    return out


def to_tolerance(op, b, n, diag, scale, alternations, maxiter):
    solvers = solvers_of(op, diag, scale)
    x = torch.zeros(n, dtype=torch.float64, device=b.device)
    res = torch.empty(n, dtype=torch.float64, device=b.device)
    found = {}
    for k in ROUTES:                                                     # the count and the status; also the warm-up
        x.zero_()
        info = solvers[k].solve(b, x, rtol=1e-10, maxiter=maxiter, check_every=64)
        solvers[k].product(x, out=res)
        found[k] = {"status": info.status, "iterations": info.iterations, "recursive_residual_over_b": info.residual / float(b.norm()),
                    "true_residual_over_b": float((b - res).norm() / b.norm())}
    ms = {k: [] for k in ROUTES}
    for _ in range(alternations):
        for k in ROUTES:
            x.zero_()
            N = max(found[k]["iterations"], 1) if found[k]["status"] == 0 else maxiter
            ms[k].append(events(lambda: solvers[k].enqueue(b, x, N, rtol=1e-10)))
            got = solvers[k].info()
            assert got.iterations == found[k]["iterations"], (k, got, found[k])
    for s in solvers.values():
        s.close()
    for k in ROUTES:
        found[k]["total_ms"] = float(np.median(ms[k]))
        found[k]["ms_all"] = [round(v, 4) for v in ms[k]]
    return {key(k): v for k, v in found.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2-2-24,3-2-40,2-4-64", help="dimension-order-neighbours, comma separated")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--maxiter", type=int, default=4000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.alternations >= 5, "at least 5 alternations"
    dev = torch.device("cuda", 0)
    record = {"device": torch.cuda.get_device_name(0), "alternations": a.alternations, "npoints": a.n, "iterations": [N1, N2],
              "maxiter": a.maxiter, "hbm_peak_GBps": bench.HBM_PEAK_GBPS,
              "method": "routes alternated in one process; HIP events around one enqueue; medians; ms per cycle (bicgstab2) or per two "
                        "iterations (bicgstab) = 2 (ms of 20 iterations - ms of 10) / 10; total_ms = enqueue of the count that solve() found "
                        "(of maxiter where it did not converge), to rtol 1e-10 from zero, stopping on the device",
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
               "per_cycle": per_cycle(op, b, n, -0.25 * h2, a.alternations), "to_rtol_1e-10": {}}
        p = rec["per_cycle"]
        print("%s n=%d | ms per cycle / two iterations %s | cycle over two iterations %s | the model's %s | over the model %s"
              % (shape, n, " ".join("%s %.4f" % (key(k), p["ms_per_cycle_or_two_iterations"][key(k)]) for k in ROUTES),
                 " ".join("%s %.3f" % kv for kv in p["cycle_over_two_iterations"].items()),
                 " ".join("%.3f" % v for v in p["model_ratio"].values()), " ".join("%.3f" % v for v in p["over_model"].values())), flush=True)
        if p["stopped_early"]:
            print("  NOT VALID: solves stopped before their iteration limit: %s" % p["stopped_early"][:4], flush=True)
        systems = [("tau1", op, 1.0, -1.0 * h2)]
        dirichlet = None
        if dim == 2:
            systems.insert(0, ("tau0.25", op, 1.0, -0.25 * h2))
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
