#!/usr/bin/env python
"""Blocks over points on coupled fields (wlsqm.hip.PointBlockJacobi) against the scalar diagonal, the route that
existed before them, on the elasticity clouds of tools/time_krylov_system.py.  The routes ALTERNATED on one GPU:
    python tools/time_krylov_system_block.py [--shapes 2-24,3-40] [--n 1000000] [--alternations 7] [--maxiter 4000]
                                             [--out profiles/krylov_system_block_timings.json]
Routes, HIP events around one enqueue each, rtol = atol = 0 so that no timed solve stops before its iteration limit:
  jacobi        StencilSystemSolver with "jacobi";
  points-P      StencilSystemSolver with PointBlockJacobi(P), P = 4 / 8 / 16 in 2D and 2 / 5 / 10 in 3D;
  flattened-R   2D only: matrix() through StencilOperator.from_coefficients, StencilSolver with BlockJacobi(R), R = 2 P.
N = 10 and N = 20; ms per iteration is the difference over 10, the start's cost what is left of the 10 (it holds the factor).
Medians of `alternations` rounds after a warm-up of every route.
The traffic model, bytes per point: a Jacobi iteration is time_krylov_system.py's 2 ((4 + 8 nop)(K + 1) + 4 + 24 m) + 152 m; the
blocks add two streams of 8 NB^2 / R bytes per flat row, 16 m NB^2 / R per point.  The expectation that DESIGN.md states ahead of the
run: ms(points-P) <= 1.15 ms(jacobi) bytes(points-P) / bytes(jacobi).
Then every system route runs once to rtol 1e-10 within `maxiter` iterations (one enqueue, no host read inside): iterations, status, ms."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "python-wlsqm_amd")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import bench  # noqa: E402
import synth  # noqa: E402
import wlsqm  # noqa: E402
import wlsqm.hip as hip  # noqa: E402
from time_krylov_system import N1, N2, SECOND, elasticity_coupling, events, flattened  # noqa: E402

POINTS = {2: (4, 8, 16), 3: (2, 5, 10)}
MARGIN = 1.15


def measure(op, S, dim, K, n, alternations, maxiter):
    dev = op._device
    m, nop = dim, len(SECOND[dim]) + 1
    coupling = elasticity_coupling(dim)
    solvers = {"jacobi": hip.StencilSystemSolver(op, coupling, diag=0.0)}
    for p in POINTS[dim]:
        solvers["points-%d" % p] = hip.StencilSystemSolver(op, coupling, diag=0.0, preconditioner=hip.PointBlockJacobi(p))
    flat_op = None
    if dim == 2:
        flat_op = flattened(solvers["jacobi"])[0]
        for p in POINTS[dim]:
            solvers["flattened-%d" % (m * p)] = hip.StencilSolver(flat_op, diag=0.0, scale=1.0, preconditioner=hip.BlockJacobi(m * p))
    b = torch.stack([torch.sin((3 + a) * S[:, 0]) * torch.cos((2 + a) * S[:, -1]) for a in range(m)], dim=1).contiguous()
    x = torch.zeros((n, m), dtype=torch.float64, device=dev)
    early = []

    def run(name, N, rtol=0.0):
        solver = solvers[name]
        flat = name.startswith("flattened")
        x.zero_()
        ms = events(lambda: solver.enqueue(b.view(-1) if flat else b, x.view(-1) if flat else x, N, rtol=rtol))
        got = solver.info()
        if rtol == 0.0 and (got.status, got.iterations) != (1, N):
            early.append((name, N, got.status, got.iterations))
        return ms, got

    for name in solvers:                                                 # the warm-up of every route
        run(name, N2); run(name, N1)
    ms = {k: {N1: [], N2: []} for k in solvers}
    for _ in range(alternations):
        for k in solvers:
            for N in (N1, N2):
                ms[k][N].append(run(k, N)[0])
    med = {k: {N: float(np.median(ms[k][N])) for N in (N1, N2)} for k in solvers}
    per_it = {k: (med[k][N2] - med[k][N1]) / (N2 - N1) for k in solvers}
    base = 2 * ((4 + 8 * nop) * (K + 1) + 4 + 24 * m) + 152 * m
    model, expectation = {"jacobi": base}, {}
    for p in POINTS[dim]:
        rows = m * p
        nb = 8 if rows <= 8 else 16 if rows <= 16 else 32
        k = "points-%d" % p
        model[k] = base + 16.0 * m * nb * nb / rows
        bound = MARGIN * per_it["jacobi"] * model[k] / base
        expectation[k] = {"bound_ms": bound, "measured_ms": per_it[k], "over_jacobi": per_it[k] / per_it["jacobi"],
                          "model_ratio": model[k] / base, "held": bool(per_it[k] <= bound)}
    to_rtol = {}
    for k in solvers:
        if not k.startswith("flattened"):
            t, got = run(k, maxiter, rtol=1e-10)
            to_rtol[k] = {"iterations": got.iterations, "status": got.status, "residual": got.residual, "ms": t}
    out = {"m": m, "nop": nop, "stopped_early": early, "ms_per_iteration": per_it, "model_bytes_per_point": model, "expectation": expectation,
           "start_ms": {k: med[k][N1] - N1 * per_it[k] for k in solvers},
           "to_rtol_1e-10": {"maxiter": maxiter, "routes": to_rtol},
           "median_ms": {k: {str(N): v for N, v in med[k].items()} for k in solvers},
           "ms_all": {k: {str(N): [round(v, 5) for v in ms[k][N]] for N in (N1, N2)} for k in solvers},
           "memory_bytes": {k: s.memory_used() for k, s in solvers.items()}}
    for s in solvers.values():
        s.close()
    if flat_op is not None:
        flat_op.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2-24,3-40", help="dimension-neighbours, comma separated")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--maxiter", type=int, default=4000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.alternations >= 5, "at least 5 alternations"
    dev = torch.device("cuda", 0)
    record = {"device": torch.cuda.get_device_name(0), "alternations": a.alternations, "iterations": [N1, N2],
              "system": "linear elasticity, lambda = mu = 1, identity rows on the 1.2 h boundary band",
              "method": "routes alternated in one process; HIP events around one enqueue; medians; ms per iteration = (ms of 20 - ms of 10) / 10",
              "baseline": "StencilSystemSolver with the scalar diagonal ('jacobi')",
              "model": "bytes per point and iteration: 2 ((4 + 8 nop)(K + 1) + 4 + 24 m) + 152 m, plus 16 m NB^2 / R with the blocks",
              "expectation": "stated before the run: ms(points-P) <= %.2f ms(jacobi) bytes(points-P) / bytes(jacobi)" % MARGIN,
              "clouds": {}}
    for shape in a.shapes.split(","):
        dim, K = (int(v) for v in shape.split("-"))
        n = a.n
        S = torch.from_numpy(synth.halton(n, dim)).to(dev)
        S = S[bench.morton_order_device(S)].contiguous()
        hoods = hip.knn(S, K)
        nk = torch.full((n,), K, dtype=torch.int32, device=dev)
        knowns = torch.full((n,), 1, dtype=torch.int64, device=dev)
        wm = torch.full((n,), wlsqm.WEIGHT_CENTER, dtype=torch.int32, device=dev)
        band = torch.minimum(S, 1.0 - S).min(dim=1).values < 1.2 * n ** (-1.0 / dim)
        d2 = hip.stencil_rows(dim, 2, *(getattr(wlsqm, "i%d_%s" % (dim, name)) for name in SECOND[dim]), device=dev)
        rows = torch.zeros((d2.shape[0] + 1, n, d2.shape[1]), dtype=torch.float64, device=dev)
        rows[:-1] = torch.where(band[None, :, None], torch.zeros((), dtype=torch.float64, device=dev), d2[:, None, :])
        rows[-1, :, 0] = band.to(torch.float64)
        op = hip.StencilOperator(dim, 2, S, hoods, nk, knowns, wm, rows)
        rec = dict(dimension=dim, order=2, nk=K, npoints=n, **measure(op, S, dim, K, n, a.alternations, a.maxiter))
        name = "%s n=%d" % (shape, n)
        record["clouds"][name] = rec
        for k, v in rec["ms_per_iteration"].items():
            e = rec["expectation"].get(k)
            r = rec["to_rtol_1e-10"]["routes"].get(k)
            print("%s | %-13s %.4f ms/iteration  start %.4f ms%s%s" % (
                name, k, v, rec["start_ms"][k],
                "" if e is None else "  bound %.4f (%s)" % (e["bound_ms"], "held" if e["held"] else "NOT held"),
                "" if r is None else "  to rtol: %d iterations, status %d, %.1f ms" % (r["iterations"], r["status"], r["ms"])), flush=True)
        if rec["stopped_early"]:
            print("  NOT VALID: solves stopped before their iteration limit: %s" % rec["stopped_early"][:4], flush=True)
        op.close()
        del S, hoods, rows, op
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
