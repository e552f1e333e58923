#!/usr/bin/env python
"""Coupled fields (wlsqm.hip.StencilSystemSolver) against the route that existed before it: the same system
flattened by matrix() and StencilOperator.from_coefficients into a scalar matrix of m n rows and iterated by StencilSolver with Jacobi.
The routes ALTERNATED on one GPU (the method of tools/time_krylov.py: a ratio is only good inside one process):
    python tools/time_krylov_system.py [--shapes 2-24,3-40] [--n 1000000] [--alternations 7] [--out profiles/krylov_system_timings.json]
Clouds: n Halton points in Morton order, K nearest neighbours, order 2, b_F known, centre weighting.  System: linear elasticity
(lambda = mu = 1), -(mu Lap u + (lambda + mu) grad div u) = f inside, identity rows on the band within 1.2 h of the boundary: the
second-derivative planes (3 in 2D, 6 in 3D) with zero rows on the band and one `value` plane that is zero inside; m = dimension,
nop = 4 or 7.  rtol = atol = 0, so that no solve stops before its iteration limit (a timed run that does not end with status 1 at
exactly N iterations is listed under stopped_early).  Routes, HIP events around each:
  fused      one StencilSystemSolver.enqueue(b, x, N);
  flattened  one StencilSolver.enqueue(b, x, N) on the flattened operator, b and x the same memory seen as (m n,).
N = 10 and N = 20; ms per iteration is the difference over 10.  Medians of `alternations` rounds after a warm-up of every route.
The traffic model, bytes per point, counted from the layout: a product reads (4 + 8 nop)(K + 1) + 4 + 24 m fused and
12 m^2 (K + 1) + 4 m + 24 m flattened; an iteration is two products and 152 m bytes of vector traffic on either route."""
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
LAMBDA = MU = 1.0
SECOND = {2: ("X2", "XY", "Y2"), 3: ("X2", "XY", "Y2", "YZ", "Z2", "XZ")}
PURE = {2: (0, 2), 3: (0, 2, 4)}
MIXED = {2: {(0, 1): 1}, 3: {(0, 1): 1, (1, 2): 3, (0, 2): 5}}


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def elasticity_coupling(dim):
    nop = len(SECOND[dim]) + 1
    cp = np.zeros((dim, dim, nop))
    for a in range(dim):
        for p in PURE[dim]:
            cp[a, a, p] -= MU
        cp[a, a, PURE[dim][a]] -= LAMBDA + MU
        cp[a, a, nop - 1] = 1.0
        for b in range(dim):
            if a != b:
                cp[a, b, MIXED[dim][min(a, b), max(a, b)]] = -(LAMBDA + MU)
    return cp


def flattened(system):
    """The scalar operator of m n rows that StencilSolver takes: matrix() row by row into from_coefficients' padded lists."""
    M = system.matrix()
    crow, col, val = M.crow_indices(), M.col_indices(), M.values()
    rows = int(crow.shape[0]) - 1
    nk = (crow[1:] - crow[:-1])
    K = int(nk.max())
    row = torch.repeat_interleave(torch.arange(rows, device=col.device), nk)
    slot = torch.arange(col.shape[0], device=col.device) - crow[:-1][row]
    hoods = torch.zeros((rows, K), dtype=torch.int32, device=col.device)
    slots = torch.zeros((1, rows, K), dtype=torch.float64, device=col.device)
    hoods[row, slot] = col.to(torch.int32)
    slots[0, row, slot] = val
    return hip.StencilOperator.from_coefficients(hoods, nk.to(torch.int32), slots, rows), int(col.shape[0])


def measure(op, S, dim, K, n, alternations):
    dev = op._device
    m, nop = dim, len(SECOND[dim]) + 1
    system = hip.StencilSystemSolver(op, elasticity_coupling(dim), diag=0.0)
    flat_op, nnz = flattened(system)
    flat = hip.StencilSolver(flat_op, diag=0.0, scale=1.0)
    b = torch.stack([torch.sin((3 + a) * S[:, 0]) * torch.cos((2 + a) * S[:, -1]) for a in range(m)], dim=1).contiguous()
    x = torch.zeros((n, m), dtype=torch.float64, device=dev)
    early = []

    def fused(N):
        x.zero_()
        ms = events(lambda: system.enqueue(b, x, N, rtol=0.0))
        got = system.info()
        if (got.status, got.iterations) != (1, N):
            early.append(("fused", N, got.status, got.iterations))
        return ms

    def flattened_route(N):
        x.zero_()
        ms = events(lambda: flat.enqueue(b.view(-1), x.view(-1), N, rtol=0.0))
        got = flat.info()
        if (got.status, got.iterations) != (1, N):
            early.append(("flattened", N, got.status, got.iterations))
        return ms

    routes = {"fused": fused, "flattened": flattened_route}
    # the routes hold the same matrix: one product of each on the same vector, to rounding.  The iterates of two unconverged BiCGSTAB
    # runs whose sums are ordered differently drift apart (recorded after 2 and after N2 iterations, not asserted)
    v = torch.randn((n, m), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    y_fused, y_flat = system.product(v)[0], flat.product(v.view(-1))[0].view(n, m)
    product_differ = float((y_fused - y_flat).abs().max() / y_fused.abs().max())
    assert product_differ <= 1e-12, "the fused and the flattened products differ by %.3e of the largest entry" % product_differ
    drift = {}
    for N in (2, N2):                                                    # N2: the warm-up of every route
        fused(N)
        ref = x.clone()
        flattened_route(N)
        drift[str(N)] = float((x - ref).abs().max() / ref.abs().max())
    fused(N1); flattened_route(N1)
    ms = {k: {N1: [], N2: []} for k in routes}
    for _ in range(alternations):
        for k, fn in routes.items():
            for N in (N1, N2):
                ms[k][N].append(fn(N))
    med = {k: {N: float(np.median(ms[k][N])) for N in (N1, N2)} for k in routes}
    per_it = {k: (med[k][N2] - med[k][N1]) / (N2 - N1) for k in routes}
    product = {"fused": (4 + 8 * nop) * (K + 1) + 4 + 24 * m, "flattened": 12 * m * m * (K + 1) + 4 * m + 24 * m}
    iteration = {k: 2 * v + 152 * m for k, v in product.items()}
    ratio = per_it["fused"] / per_it["flattened"]
    out = {"m": m, "nop": nop, "stored_entries_per_point": op._m["total"] / n, "flattened_stored_entries_per_point": flat_op._m["total"] / n,
           "flattened_nonzeros": nnz, "stopped_early": early, "products_differ_by": product_differ, "iterates_differ_by": drift,
           "ms_per_iteration": per_it, "ratio_fused_over_flattened": ratio,
           "model_bytes_per_point": {"product": product, "iteration": iteration},
           "model_ratio_product": product["fused"] / product["flattened"], "model_ratio_iteration": iteration["fused"] / iteration["flattened"],
           "over_product_model": ratio / (product["fused"] / product["flattened"]),
           "over_iteration_model": ratio / (iteration["fused"] / iteration["flattened"]),
           "start_ms": {k: med[k][N1] - N1 * per_it[k] for k in routes},
           "median_ms": {k: {str(N): v for N, v in med[k].items()} for k in routes},
           "ms_all": {k: {str(N): [round(v, 5) for v in ms[k][N]] for N in (N1, N2)} for k in routes},
           "memory_bytes": {"fused_solver": system.memory_used(), "flattened_solver": flat.memory_used(), "operator": op.memory_used(),
                            "flattened_operator": flat_op.memory_used()}}
    system.close(); flat.close(); flat_op.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2-24,3-40", help="dimension-neighbours, comma separated")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.alternations >= 5, "at least 5 alternations"
    dev = torch.device("cuda", 0)
    record = {"device": torch.cuda.get_device_name(0), "alternations": a.alternations, "iterations": [N1, N2],
              "system": "linear elasticity, lambda = mu = 1, identity rows on the 1.2 h boundary band; no stop before the iteration limit",
              "method": "routes alternated in one process; HIP events around one enqueue; medians; ms per iteration = (ms of 20 - ms of 10) / 10",
              "baseline": "matrix() flattened through StencilOperator.from_coefficients, iterated by StencilSolver with Jacobi",
              "model": "bytes per point: product fused (4 + 8 nop)(K + 1) + 4 + 24 m, flattened 12 m^2 (K + 1) + 28 m; iteration = 2 products + 152 m",
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
        rec = dict(dimension=dim, order=2, nk=K, npoints=n, **measure(op, S, dim, K, n, a.alternations))
        name = "%s n=%d" % (shape, n)
        record["clouds"][name] = rec
        p = rec["ms_per_iteration"]
        print("%s | fused %.4f ms/iteration  flattened %.4f  ratio %.3f  model: product %.3f iteration %.3f  over them %.3f %.3f"
              % (name, p["fused"], p["flattened"], rec["ratio_fused_over_flattened"], rec["model_ratio_product"], rec["model_ratio_iteration"],
                 rec["over_product_model"], rec["over_iteration_model"]), flush=True)
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
