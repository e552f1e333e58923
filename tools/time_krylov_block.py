#!/usr/bin/env python
"""The block-Jacobi preconditioner of wlsqm.hip.StencilSolver (BlockJacobi) against the Jacobi route of the same
process and commit, the routes ALTERNATED on one GPU (the method of tools/time_krylov.py: a ratio is only good inside one process):
    python tools/time_krylov_block.py [--shapes 2-2-24,3-2-40,2-4-64] [--n 1000000] [--alternations 7] [--maxiter 4000]
                                      [--out profiles/krylov_block_timings.json]
Clouds: those of tools/time_krylov.py (n Halton points in Morton order, K nearest neighbours, b_F known, centre weighting).
Routes: "jacobi" and BlockJacobi(8), (16), (32), each its own solver on the one operator; HIP events around one enqueue; medians of
`alternations` rounds after a warm-up of every route.
  1. per iteration, every cloud: (I - 0.25 h^2 Lap_h) x = b with rtol = atol = 0, N = 10 and N = 20 iterations; ms per iteration is the
     difference over 10, start_ms what is left of the N = 10 run (the factor of the blocks or the diagonal, the first residual).  A timed
     run that does not end with status 1 at exactly N iterations is listed under stopped_early.  The traffic model of section 17 (2
     passes over 12 bytes per stored entry, 25 vector accesses of 8 bytes and 2 of 4 per point) gains two streams of 8 * block bytes
     per point; `over_model` is a route's ms per iteration over Jacobi's scaled by that byte ratio (section 19 expects <= 1.15).
  2. to rtol 1e-10 from zero, the 2D clouds: I - tau h^2 Lap_h at tau 0.25 and 1, and the Dirichlet Poisson problem (-Lap_h inside,
     identity rows within 1.2 h of the boundary).  One solve() finds the count and the status; the timed call is enqueue(b, x, count),
     which stops on the device with no host read.  A route that does not converge within --maxiter is reported with its status and the
     time of its --maxiter iterations."""
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
ROUTES = ("jacobi", "block8", "block16", "block32")


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def solvers_of(op, diag, scale):
    out = {"jacobi": hip.StencilSolver(op, diag=diag, scale=scale)}
    for nb in (8, 16, 32):
        out["block%d" % nb] = hip.StencilSolver(op, diag=diag, scale=scale, preconditioner=hip.BlockJacobi(nb))
    return out


def per_iteration(op, b, n, scale, alternations):
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
                    early.append((k, N, got.status, got.iterations))
    med = {k: {N: float(np.median(v)) for N, v in ms[k].items()} for k in ROUTES}
    per_it = {k: (med[k][N2] - med[k][N1]) / (N2 - N1) for k in ROUTES}
    start = {k: med[k][N1] - N1 * per_it[k] for k in ROUTES}
    total = op._m["total"]
    model = {"jacobi": 2 * total * (4 + 8) + n * (25 * 8 + 2 * 4)}
    for nb in (8, 16, 32):
        model["block%d" % nb] = model["jacobi"] + n * 2 * 8 * nb
    over = {k: per_it[k] / (per_it["jacobi"] * model[k] / model["jacobi"]) for k in ROUTES}
    mem = {k: s.memory_used() for k, s in solvers.items()}
    for s in solvers.values():
        s.close()
    return {"ms_per_iteration": per_it, "start_ms": start, "median_ms": {k: {str(N): v for N, v in med[k].items()} for k in med},
            "ms_all": {k: {str(N): [round(v, 5) for v in vs] for N, vs in ms[k].items()} for k in ms},
            "traffic_model_bytes_per_iteration": model, "model_ratio_to_jacobi": {k: model[k] / model["jacobi"] for k in ROUTES},
            "ratio_to_jacobi": {k: per_it[k] / per_it["jacobi"] for k in ROUTES}, "over_model": over,
            "hbm_frac": {k: model[k] / (per_it[k] * 1e-3) / (bench.HBM_PEAK_GBPS * 1e9) for k in ROUTES},
            "stopped_early": early, "solver_memory_bytes": mem}


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
            N = max(found[k]["iterations"], 1)
            ms[k].append(events(lambda: solvers[k].enqueue(b, x, N, rtol=1e-10)))
            got = solvers[k].info()
            assert got.iterations == found[k]["iterations"], (k, got, found[k])
    for s in solvers.values():
        s.close()
    for k in ROUTES:
        found[k]["total_ms"] = float(np.median(ms[k]))
        found[k]["ms_all"] = [round(v, 4) for v in ms[k]]
    return found


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
              "method": "routes alternated in one process; HIP events around one enqueue; medians; ms per iteration = (ms of 20 - ms of 10) / 10; "
                        "total_ms = enqueue of the count that solve() found, to rtol 1e-10 from zero, stopping on the device",
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
               "per_iteration": per_iteration(op, b, n, -0.25 * h2, a.alternations), "to_rtol_1e-10": {}}
        p = rec["per_iteration"]
        print("%s n=%d | ms/iteration %s | over Jacobi %s | over the model %s | start ms %s"
              % (shape, n, " ".join("%s %.4f" % (k, p["ms_per_iteration"][k]) for k in ROUTES),
                 " ".join("%.3f" % p["ratio_to_jacobi"][k] for k in ROUTES), " ".join("%.3f" % p["over_model"][k] for k in ROUTES),
                 " ".join("%.3f" % p["start_ms"][k] for k in ROUTES)), flush=True)
        if p["stopped_early"]:
            print("  NOT VALID: solves stopped before their iteration limit: %s" % p["stopped_early"][:4], flush=True)
        if dim == 2:
            systems = [("tau0.25", op, 1.0, -0.25 * h2), ("tau1", op, 1.0, -1.0 * h2)]
            band = (torch.minimum(S, 1.0 - S).min(dim=1).values < 1.2 * n ** (-1.0 / dim))
            e_f = hip.stencil_rows(dim, order, "value", device=dev)
            rows = torch.where(band[:, None], e_f[0][None, :], -lap[0][None, :])[None].contiguous()
            dirichlet = hip.StencilOperator(dim, order, S, hoods, nk, knowns, wm, rows)
            systems.append(("dirichlet", dirichlet, 0.0, 1.0))
            for what, sys_op, diag, scale in systems:
                found = to_tolerance(sys_op, b, n, diag, scale, a.alternations, a.maxiter)
                rec["to_rtol_1e-10"][what] = found
                print("  %s to rtol 1e-10 | %s" % (what, " | ".join("%s %d its (status %d) %.2f ms, true %.1e"
                      % (k, found[k]["iterations"], found[k]["status"], found[k]["total_ms"], found[k]["true_residual_over_b"]) for k in ROUTES)),
                      flush=True)
            dirichlet.close()
            del dirichlet, rows, band
        record["shapes"][shape] = rec
        op.close()
        del S, hoods, b, op
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
