#!/usr/bin/env python
"""Stacked right-hand sides (wlsqm.hip.StencilSolver(nfields=R).enqueue_many) against R sequential single-field
enqueues of the same process, the routes ALTERNATED on one GPU (the method of tools/time_krylov.py: a ratio is only good inside one process):
    python tools/time_krylov_many.py [--shapes 2-2-24,3-2-40,2-4-64] [--n 1000000] [--small 10000] [--alternations 7]
                                     [--out profiles/krylov_many_timings.json]
Clouds: those of tools/time_krylov.py (n Halton points in Morton order, K nearest neighbours, b_F known, centre weighting), and the first
shape once more on --small points, where an iteration is eight launch latencies.  System: (I - 0.25 h^2 Lap_h) x_f = b_f with rtol = atol
= 0, so that no field stops before its iteration limit (a timed run that does not end with status 1 at exactly N iterations in every field is
listed under stopped_early).  Preconditioners "jacobi" and BlockJacobi(16); R = 2, 4, 8.  Routes, HIP events around each:
  stacked   one enqueue_many(b, x, N) of a solver with nfields = R;
  singles   R enqueue(b[f], x[f], N) in a row on a solver with nfields = 1: the single-field kernels, which this feature leaves as they were.
N = 10 and N = 20; ms per iteration is the difference over 10.  Medians of `alternations` rounds after a warm-up of every route.
The traffic model, bytes per point and iteration with e stored entries per row and nb the block size (0 for Jacobi): the single solve
24 e + 208 + 16 nb (section 17, 19), the stacked one 24 e + 8 + 200 R + 16 nb: the matrix, len and the block plane once, the 25 vector
accesses per field.  `over_model` is the measured ratio stacked / singles over the model's.
With --compare, the singles' ms per iteration over R (Jacobi, R = 2) is set beside the ms per iteration of earlier records of
tools/time_krylov.py ("a_eager") or tools/time_krylov_block.py ("jacobi") for the same shape."""
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
FIELDS = (2, 4, 8)
PRECONDITIONERS = {"jacobi": 0, "block16": 16}


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def measure(op, B, n, scale, alternations):
    """The record of one cloud: B (8, n), the right-hand sides."""
    dev = B.device
    X = torch.zeros((8, n), dtype=torch.float64, device=dev)
    pre = lambda nb: hip.BlockJacobi(nb) if nb else "jacobi"
    ones = {p: hip.StencilSolver(op, diag=1.0, scale=scale, preconditioner=pre(nb)) for p, nb in PRECONDITIONERS.items()}
    many = {(p, R): hip.StencilSolver(op, diag=1.0, scale=scale, preconditioner=pre(nb), nfields=R)
            for p, nb in PRECONDITIONERS.items() for R in FIELDS}
    early = []

    def stacked(p, R, N):
        X.zero_()
        ms = events(lambda: many[p, R].enqueue_many(B[:R], X[:R], N, rtol=0.0))
        for f, got in enumerate(many[p, R].info_many()):
            if (got.status, got.iterations) != (1, N):
                early.append(("stacked", p, R, N, f, got.status, got.iterations))
        return ms

    def singles(p, R, N):
        X.zero_()

        def run():
            for f in range(R):
                ones[p].enqueue(B[f], X[f], N, rtol=0.0)
        ms = events(run)
        got = ones[p].info()
        if (got.status, got.iterations) != (1, N):
            early.append(("singles", p, R, N, R - 1, got.status, got.iterations))
        return ms

    routes = {"stacked": stacked, "singles": singles}
    cells = [(p, R) for p in PRECONDITIONERS for R in FIELDS]
    for p, R in cells:                                                   # warm-up of every route, and: the routes compute the same solves
        singles(p, R, N2)
        ref = X[:R].clone()
        stacked(p, R, N2)
        assert torch.equal(X[:R].view(torch.int64), ref.view(torch.int64)), "stacked and single solves differ: %s R = %d" % (p, R)
        stacked(p, R, N1); singles(p, R, N1)
    ms = {(k, p, R): {N1: [], N2: []} for k in routes for p, R in cells}
    for _ in range(alternations):
        for p, R in cells:
            for k, fn in routes.items():
                for N in (N1, N2):
                    ms[k, p, R][N].append(fn(p, R, N))
    e = op._m["total"] / n
    out = {"stored_entries_per_row": e, "cells": {}, "stopped_early": early,
           "solver_memory_bytes": {"one": {p: s.memory_used() for p, s in ones.items()},
                                   "stacked": {"%s R=%d" % k: s.memory_used() for k, s in many.items()}}}
    for p, R in cells:
        med = {k: {N: float(np.median(ms[k, p, R][N])) for N in (N1, N2)} for k in routes}
        per_it = {k: (med[k][N2] - med[k][N1]) / (N2 - N1) for k in routes}
        nb = PRECONDITIONERS[p]
        model = (24 * e + 8 + 200 * R + 16 * nb) / (R * (24 * e + 208 + 16 * nb))
        ratio = per_it["stacked"] / per_it["singles"]
        out["cells"]["%s R=%d" % (p, R)] = {
            "ms_per_iteration": {"stacked": per_it["stacked"], "R_singles": per_it["singles"], "one_single": per_it["singles"] / R},
            "ratio_stacked_over_singles": ratio, "model_ratio": model, "over_model": ratio / model,
            "start_ms": {k: med[k][N1] - N1 * per_it[k] for k in routes},
            "median_ms": {k: {str(N): v for N, v in med[k].items()} for k in routes},
            "ms_all": {k: {str(N): [round(v, 5) for v in ms[k, p, R][N]] for N in (N1, N2)} for k in routes}}
    for s in list(ones.values()) + list(many.values()):
        s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2-2-24,3-2-40,2-4-64", help="dimension-order-neighbours, comma separated")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--small", type=int, default=10_000, help="points of the launch-bound cloud of the first shape (0: none)")
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--compare", nargs="*", default=[], help="records of tools/time_krylov.py (a_eager) or tools/time_krylov_block.py "
                    "(jacobi): their ms per iteration beside this run's nfields = 1 time")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.alternations >= 5, "at least 5 alternations"
    dev = torch.device("cuda", 0)
    record = {"device": torch.cuda.get_device_name(0), "alternations": a.alternations, "iterations": [N1, N2], "fields": list(FIELDS),
              "system": "I - 0.25 h^2 Laplacian per field, no stop before the iteration limit",
              "method": "routes alternated in one process; HIP events around one enqueue_many (stacked) or R enqueues in a row (singles, "
                        "the nfields = 1 solver); medians; ms per iteration = (ms of 20 - ms of 10) / 10",
              "model": "bytes per point and iteration: single 24 e + 208 + 16 nb, stacked 24 e + 8 + 200 R + 16 nb",
              "clouds": {}}
    earlier = {os.path.basename(f): json.load(open(f))["shapes"] for f in a.compare}
    shapes = a.shapes.split(",")
    work = [(shape, a.n) for shape in shapes] + ([(shapes[0], a.small)] if a.small else [])
    for shape, n in work:
        dim, order, K = (int(v) for v in shape.split("-"))
        S = torch.from_numpy(synth.halton(n, dim)).to(dev)
        S = S[bench.morton_order_device(S)].contiguous()
        hoods = hip.knn(S, K)
        nk = torch.full((n,), K, dtype=torch.int32, device=dev)
        knowns = torch.full((n,), 1, dtype=torch.int64, device=dev)
        wm = torch.full((n,), wlsqm.WEIGHT_CENTER, dtype=torch.int32, device=dev)
        op = hip.StencilOperator(dim, order, S, hoods, nk, knowns, wm, hip.stencil_rows(dim, order, "laplacian", device=dev))
        B = torch.stack([torch.sin((3 + f) * S[:, 0]) * torch.cos((2 + f) * S[:, -1]) for f in range(8)]).contiguous()
        rec = dict(dimension=dim, order=order, nk=K, npoints=n, **measure(op, B, n, -0.25 * n ** (-2.0 / dim), a.alternations))
        name = "%s n=%d" % (shape, n)
        for source, shapes_then in earlier.items():
            if shape in shapes_then and shapes_then[shape]["npoints"] == n:
                r = shapes_then[shape]
                then = r["per_iteration"]["ms_per_iteration"]["jacobi"] if "per_iteration" in r else r["ms_per_iteration"]["a_eager"]
                now = rec["cells"]["jacobi R=2"]["ms_per_iteration"]["one_single"]
                rec.setdefault("nfields_1_against_earlier_records", {})[source] = {"earlier_ms_per_iteration": then, "ms_per_iteration": now,
                                                                                  "ratio": now / then}
                print("%s | nfields = 1, Jacobi: %.4f ms per iteration, %s %.4f, ratio %.3f" % (name, now, source, then, now / then), flush=True)
        record["clouds"][name] = rec
        for cell, c in rec["cells"].items():
            m = c["ms_per_iteration"]
            print("%s | %-12s stacked %.4f ms/iteration  R singles %.4f  ratio %.3f  model %.3f  over the model %.3f"
                  % (name, cell, m["stacked"], m["R_singles"], c["ratio_stacked_over_singles"], c["model_ratio"], c["over_model"]), flush=True)
        if rec["stopped_early"]:
            print("  NOT VALID: solves stopped before their iteration limit: %s" % rec["stopped_early"][:4], flush=True)
        op.close()
        del S, hoods, B, op
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
