#!/usr/bin/env python
"""wlsqm.hip.SpatialOrder: what building the order costs, what "order-relabel" reaches, and what a user whose
cloud comes in random order buys with it.  Routes ALTERNATED in one process on one GPU, HIP events, medians of `alternations` rounds
after a warm-up of every route (the method of tools/time_krylov.py):
    python tools/time_order.py [--n 1000000] [--alternations 7] [--shapes 2-2-24,3-2-40,2-4-64] [--maxiter 4000]
                               [--out profiles/order_timings.json]
Clouds: n Halton points, SHUFFLED (seeded), K nearest neighbours, b_F known, centre weighting.
  a. building the order, 2D and 3D: SpatialOrder(S) (bounding box, "order-keys", hipcub's radix sort of 64-bit pairs, "order-inverse",
     two host synchronisations) against bench.morton_order_device(S), the torch route: 16 bits per axis, 32 or 48 passes and argsort.
  b. "order-relabel", 1M rows at K = 24 / 40 / 64: order.hoods(hoods, check=False, out=) against the torch expression
     inverse[hoods[perm].long()].  Model: 8 K + 4 bytes streamed per row (the list read and written, the row's number), 4 K bytes
     gathered from the 4 n-byte inverse table; reported: the streamed bytes over the time, as a fraction of the HBM peak.
  c. per shape, as given against reordered (order.cloud, so the same neighbourhoods) and against the control "morton16" (the same points
     ordered by bench.morton_order_device and searched again: the order of every other tool's clouds): fit_cloud_device, op.apply (Laplacian, one
     field), one StencilSolver iteration with "jacobi" and with BlockJacobi(16) (the difference of 20 and 10 iterations), and the
     iterations and total ms of (I - h^2 Lap_h) x = b to rtol 1e-10 with BlockJacobi(16) and method="bicgstab2"."""
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
NDOF = {2: (1, 3, 6, 10, 15), 3: (1, 4, 10, 20, 35)}


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(routes, alternations):
    """{name: (median ms, all ms)} of the callables in `routes`, one after the other in every round, after one warm-up of each."""
    for fn in routes.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in routes}
    for _ in range(alternations):
        for k, fn in routes.items():
            ms[k].append(events(fn))
    return {k: {"median_ms": float(np.median(v)), "ms_all": [round(t, 5) for t in v]} for k, v in ms.items()}


def shuffled_cloud(n, dim, dev):
    S = synth.halton(n, dim)
    return torch.from_numpy(np.ascontiguousarray(S[np.random.default_rng([11, n, dim]).permutation(n)])).to(dev)


def build_order(n, dim, dev, alternations):
    S = shuffled_cloud(n, dim, dev)
    got = alternate({"SpatialOrder": lambda: hip.SpatialOrder(S), "torch_16_bits": lambda: bench.morton_order_device(S)}, alternations)
    got["SpatialOrder_over_torch"] = got["SpatialOrder"]["median_ms"] / got["torch_16_bits"]["median_ms"]
    return got


def relabel(n, dev, alternations):
    S = shuffled_cloud(n, 2, dev)
    order = hip.SpatialOrder(S)
    out = {}
    for K in (24, 40, 64):
        hoods = torch.randint(0, n, (n, K), dtype=torch.int32, device=dev)
        dst = torch.empty_like(hoods)
        got = alternate({"order-relabel": lambda: order.hoods(hoods, check=False, out=dst),
                         "torch": lambda: order.inverse[hoods[order.perm].long()]}, alternations)
        assert torch.equal(dst.long(), order.inverse[hoods[order.perm].long()])
        streamed = n * (8 * K + 4)
        gbps = streamed / (got["order-relabel"]["median_ms"] * 1e-3) / 1e9
        got.update(streamed_bytes=streamed, gathered_bytes=4 * K * n, table_bytes=4 * n, streamed_GBps=gbps,
                   fraction_of_hbm_peak=gbps / bench.HBM_PEAK_GBPS,
                   relabel_over_torch=got["order-relabel"]["median_ms"] / got["torch"]["median_ms"])
        out[str(K)] = got
        del hoods, dst
    return out


def user_buys(shape, n, dev, alternations, maxiter):
    dim, order_, K = (int(v) for v in shape.split("-"))
    S = shuffled_cloud(n, dim, dev)
    geo = (S, hip.knn(S, K), torch.full((n,), K, dtype=torch.int32, device=dev), torch.full((n,), 1, dtype=torch.int64, device=dev),
           torch.full((n,), wlsqm.WEIGHT_CENTER, dtype=torch.int32, device=dev))
    order = hip.SpatialOrder(S)
    # the control: the same points ordered by the torch route that bench.py carries (16 bits per axis), searched again
    S16 = S[bench.morton_order_device(S)].contiguous()
    clouds = {"as_given": geo, "reordered": order.cloud(*geo), "morton16": (S16, hip.knn(S16, K)) + geo[2:]}
    lap = hip.stencil_rows(dim, order_, "laplacian", device=dev)
    h2 = n ** (-2.0 / dim)
    no = NDOF[dim][order_]
    F0 = torch.sin(3 * S[:, 0]) * torch.cos(2 * S[:, -1])
    Fs = {"as_given": F0, "reordered": order.take(F0).contiguous(), "morton16": torch.sin(3 * S16[:, 0]) * torch.cos(2 * S16[:, -1])}
    fi = torch.zeros((n, no), dtype=torch.float64, device=dev)
    y = torch.empty((1, n), dtype=torch.float64, device=dev)
    x = torch.zeros(n, dtype=torch.float64, device=dev)
    ops = {k: hip.StencilOperator(dim, order_, *g, lap) for k, g in clouds.items()}
    rec = {"dimension": dim, "order": order_, "nk": K, "npoints": n}
    routes = {}
    for k, g in clouds.items():
        routes["fit/" + k] = lambda g=g, k=k: hip.fit_cloud_device(dim, order_, g[0], Fs[k], g[1], fi, g[2], g[3], g[4])
        routes["apply/" + k] = lambda k=k: ops[k].apply(Fs[k], out=y)
    rec["fit_and_apply"] = alternate(routes, alternations)
    solvers = {(pc, k): hip.StencilSolver(ops[k], diag=1.0, scale=-0.25 * h2, preconditioner=(pc if pc == "jacobi" else hip.BlockJacobi(16, refresh=False)))
               for pc in ("jacobi", "block16") for k in clouds}

    def run(key, N):
        x.zero_()
        solvers[key].enqueue(Fs[key[1]], x, N, rtol=0.0)

    its = alternate({"%s/%s/%d" % (pc, k, N): (lambda pc=pc, k=k, N=N: run((pc, k), N)) for (pc, k) in solvers for N in (N1, N2)}, alternations)
    rec["ms_per_iteration"] = {"%s/%s" % key: (its["%s/%s/%d" % (key + (N2,))]["median_ms"] - its["%s/%s/%d" % (key + (N1,))]["median_ms"]) / (N2 - N1)
                               for key in solvers}
    rec["iteration_runs"] = its
    for s in solvers.values():
        s.close()
    # to rtol 1e-10: one solve() finds the count and the status, the timed call is enqueue of that count
    big = {k: hip.StencilSolver(ops[k], diag=1.0, scale=-1.0 * h2, preconditioner=hip.BlockJacobi(16), method="bicgstab2") for k in clouds}
    found = {}
    for k, s in big.items():
        x.zero_()
        info = s.solve(Fs[k], x, rtol=1e-10, maxiter=maxiter, check_every=64)
        found[k] = {"status": info.status, "iterations": info.iterations}
    timed = {k: (lambda k=k: (x.zero_(), big[k].enqueue(Fs[k], x, max(found[k]["iterations"], 1), rtol=1e-10))) for k in clouds}
    tot = alternate({k: fn for k, fn in timed.items() if found[k]["status"] == 0}, alternations)
    for k in clouds:
        if found[k]["status"] != 0:                                      # a run to the iteration limit is timed once
            tot[k] = {"median_ms": events(timed[k]), "ms_all": []}
        found[k].update(total_ms=tot[k]["median_ms"], ms_all=tot[k]["ms_all"])
    rec["tau1_block16_bicgstab2_to_rtol_1e-10"] = found
    for s in big.values():
        s.close()
    for o in ops.values():
        o.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--shapes", default="2-2-24,3-2-40,2-4-64", help="dimension-order-neighbours, comma separated")
    ap.add_argument("--maxiter", type=int, default=4000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.alternations >= 5, "at least 5 alternations"
    dev = torch.device("cuda", 0)
    record = {"device": torch.cuda.get_device_name(0), "alternations": a.alternations, "npoints": a.n, "hbm_peak_GBps": bench.HBM_PEAK_GBPS,
              "method": "routes alternated in one process; HIP events around one call; medians; ms per iteration from the difference of "
                        "20 and 10 iterations with refresh=False; total_ms = enqueue of the count that solve() found, to rtol 1e-10 from zero",
              "command": "python tools/time_order.py --n %d --alternations %d --shapes %s" % (a.n, a.alternations, a.shapes)}

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(record, f, indent=1)
                f.write("\n")

    record["build"] = {}
    for dim in (2, 3):
        b = record["build"]["%dD" % dim] = build_order(a.n, dim, dev, a.alternations)
        print("build %dD n=%d | SpatialOrder %.3f ms, torch (16 bits) %.3f ms, ratio %.3f"
              % (dim, a.n, b["SpatialOrder"]["median_ms"], b["torch_16_bits"]["median_ms"], b["SpatialOrder_over_torch"]), flush=True)
    save()
    record["relabel"] = relabel(a.n, dev, a.alternations)
    for K, r in record["relabel"].items():
        print("relabel K=%s | order-relabel %.4f ms (%.0f GB/s streamed, %.2f of the HBM peak), torch %.4f ms, ratio %.3f"
              % (K, r["order-relabel"]["median_ms"], r["streamed_GBps"], r["fraction_of_hbm_peak"], r["torch"]["median_ms"], r["relabel_over_torch"]),
              flush=True)
    save()
    record["shapes"] = {}
    for shape in a.shapes.split(","):
        rec = record["shapes"][shape] = user_buys(shape, a.n, dev, a.alternations, a.maxiter)
        fa, it, tt = rec["fit_and_apply"], rec["ms_per_iteration"], rec["tau1_block16_bicgstab2_to_rtol_1e-10"]
        three = ("as_given", "reordered", "morton16")
        print("%s, as given -> reordered (bench.morton_order_device's order) | fit %s ms | apply %s ms | jacobi iteration %s ms | block16 "
              "iteration %s ms | tau 1 to 1e-10: %s"
              % (shape, "%.4f -> %.4f (%.4f)" % tuple(fa["fit/" + k]["median_ms"] for k in three),
                 "%.4f -> %.4f (%.4f)" % tuple(fa["apply/" + k]["median_ms"] for k in three),
                 "%.4f -> %.4f (%.4f)" % tuple(it["jacobi/" + k] for k in three), "%.4f -> %.4f (%.4f)" % tuple(it["block16/" + k] for k in three),
                 " -> ".join("%d its (status %d) %.2f ms" % (tt[k]["iterations"], tt[k]["status"], tt[k]["total_ms"]) for k in three)), flush=True)
        save()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
