#!/usr/bin/env python
"""Coupled fields with a per-point coupling (wlsqm.hip.StencilSystemSolver with a device tensor (m, m, nop, npoints), DESIGN.md section
26) against two routes that existed before it, forward and transposed.  The routes ALTERNATED on one GPU (the method of
tools/time_krylov_system.py, whose clouds, system and protocol these are):
    python tools/time_krylov_system_point.py [--shapes 2-24,3-40] [--n 1000000] [--alternations 7] [--out profiles/krylov_system_point_timings.json]
Routes, HIP events around each, N = 10 and N = 20 iterations, ms per iteration the difference over 10, forward and with transpose=True:
  point      StencilSystemSolver with the constant elasticity table expanded per point (the code under test);
  constant   StencilSystemSolver with the constant host table on the same operator (section 24's fused route);
  flattened  the same per-point system flattened by matrix() into a scalar matrix of m n rows and iterated by StencilSolver.
The run asserts that one product of each route on one vector agrees to 1e-12 of the largest entry, forward and transposed.
The traffic model, bytes per point and product: the constant route reads (4 + 8 nop)(K + 1) + 4 + 24 m; the per-point forward product
adds its 8 m^2 nop bytes of coefficients; the transposed one adds them in the mix, which also reads 8 m and writes 8 m nop, and the
mixed product gathers 8 m nop bytes per entry where the constant one gathers 8 m (the gathers are counted on neither side)."""
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


def measure(op, S, dim, K, n, alternations):
    dev = op._device
    m, nop = dim, len(SECOND[dim]) + 1
    cp = elasticity_coupling(dim)
    table = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(cp[..., None], cp.shape + (n,)))).to(dev)
    point = hip.StencilSystemSolver(op, table, diag=0.0)
    constant = hip.StencilSystemSolver(op, cp, diag=0.0)
    flat_op, nnz = flattened(point)
    flat = hip.StencilSolver(flat_op, diag=0.0, scale=1.0)
    for s in (point, constant, flat):
        s.prepare_transpose()
    b = torch.stack([torch.sin((3 + a) * S[:, 0]) * torch.cos((2 + a) * S[:, -1]) for a in range(m)], dim=1).contiguous()
    x = torch.zeros((n, m), dtype=torch.float64, device=dev)
    early = []

    def route(name, solver, flatten, transpose):
        def run(N):
            x.zero_()
            bb, xx = (b.view(-1), x.view(-1)) if flatten else (b, x)
            ms = events(lambda: solver.enqueue(bb, xx, N, rtol=0.0, transpose=transpose))
            got = solver.info()
            if (got.status, got.iterations) != (1, N):
                early.append((name, N, got.status, got.iterations))
            return ms
        return run

    routes = {}
    for tr in (False, True):
        for name, solver, flatten in (("point", point, False), ("constant", constant, False), ("flattened", flat, True)):
            key = name + ("_transposed" if tr else "")
            routes[key] = route(key, solver, flatten, tr)
    v = torch.randn((n, m), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    differ = {}
    for tr in (False, True):
        y = point.product(v, transpose=tr)[0]
        for name, other in (("constant", constant.product(v, transpose=tr)[0]), ("flattened", flat.product(v.view(-1), transpose=tr)[0].view(n, m))):
            d = float((y - other).abs().max() / y.abs().max())
            differ[name + ("_transposed" if tr else "")] = d
            assert d <= 1e-12, "the per-point and the %s%s products differ by %.3e of the largest entry" % (name, " transposed" if tr else "", d)
    for fn in routes.values():                                           # the warm-up of every route
        fn(N2); fn(N1)
    ms = {k: {N1: [], N2: []} for k in routes}
    for _ in range(alternations):
        for k, fn in routes.items():
            for N in (N1, N2):
                ms[k][N].append(fn(N))
    med = {k: {N: float(np.median(ms[k][N])) for N in (N1, N2)} for k in routes}
    per_it = {k: (med[k][N2] - med[k][N1]) / (N2 - N1) for k in routes}
    base = (4 + 8 * nop) * (K + 1) + 4 + 24 * m
    product = {"constant": base, "point": base + 8 * m * m * nop, "point_transposed": base + 8 * m * m * nop + 8 * m + 8 * m * nop,
               "flattened": 12 * m * m * (K + 1) + 4 * m + 24 * m}
    model = {"point_over_constant": product["point"] / product["constant"],
             "point_transposed_over_constant": product["point_transposed"] / product["constant"],
             "gathered_bytes_per_entry": {"constant": 8 * m, "point": 8 * m, "point_transposed": 8 * m * nop}}
    ratio = {"point_over_constant": per_it["point"] / per_it["constant"], "point_over_flattened": per_it["point"] / per_it["flattened"],
             "point_transposed_over_constant_transposed": per_it["point_transposed"] / per_it["constant_transposed"],
             "point_transposed_over_flattened_transposed": per_it["point_transposed"] / per_it["flattened_transposed"],
             "point_transposed_over_point": per_it["point_transposed"] / per_it["point"]}
    out = {"m": m, "nop": nop, "stored_entries_per_point": op._m["total"] / n, "flattened_nonzeros": nnz, "stopped_early": early,
           "products_differ_by": differ, "ms_per_iteration": per_it, "ratio": ratio, "model_bytes_per_point_and_product": product,
           "model": model, "forward_over_model": ratio["point_over_constant"] / model["point_over_constant"],
           "expectation_forward_at_most": 1.15,
           "median_ms": {k: {str(N): t for N, t in med[k].items()} for k in routes},
           "ms_all": {k: {str(N): [round(t, 5) for t in ms[k][N]] for N in (N1, N2)} for k in routes},
           "memory_bytes": {"point_solver": point.memory_used(), "constant_solver": constant.memory_used(), "coupling_tensor": table.numel() * 8,
                            "flattened_solver": flat.memory_used(), "operator": op.memory_used(), "flattened_operator": flat_op.memory_used()}}
    point.close(); constant.close(); flat.close(); flat_op.close()
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
              "system": "linear elasticity, lambda = mu = 1 expanded per point, identity rows on the 1.2 h boundary band; no stop before the iteration limit",
              "method": "routes alternated in one process; HIP events around one enqueue; medians; ms per iteration = (ms of 20 - ms of 10) / 10",
              "baselines": "the constant-table fused route on the same operator; matrix() of the per-point system flattened and iterated by StencilSolver",
              "model": "bytes per point and product: constant (4 + 8 nop)(K + 1) + 4 + 24 m; per-point forward + 8 m^2 nop; transposed + 8 m^2 nop + 8 m + 8 m nop",
              "clouds": {}}
    for shape in a.shapes.split(","):
        dim, K = (int(t) for t in shape.split("-"))
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
        p, r = rec["ms_per_iteration"], rec["ratio"]
        print("%s | ms/iteration point %.4f constant %.4f flattened %.4f | transposed %.4f %.4f %.4f | point / constant %.3f (model %.3f, "
              "over it %.3f), transposed %.3f" % (name, p["point"], p["constant"], p["flattened"], p["point_transposed"], p["constant_transposed"],
                                                 p["flattened_transposed"], r["point_over_constant"], rec["model"]["point_over_constant"],
                                                 rec["forward_over_model"], r["point_transposed_over_constant_transposed"]), flush=True)
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
