#!/usr/bin/env python
"""The stencil operators against the other routes to the same numbers, ALTERNATED in one process on one GPU (the boxes of a pool differ
by several per cent: a ratio is only good inside one process):
    python tools/time_stencil.py [--shapes 2-2-24,3-2-40,2-4-64] [--n 1000000] [--alternations 7] [--out profiles/stencil_timings.json]
Clouds: n Halton points in Morton order, the K nearest neighbours of each (wlsqm.hip.knn), the function value known (b_F), centre
weighting: the index-based shapes of the README.  Routes, HIP events around REPS back-to-back calls:
  apply/nop1/R1, R4   StencilOperator.apply, one operator (the Laplacian), one field and a stack of four (4, npoints);
  apply/nopG/R1, R4   the same with the gradient and the Laplacian (3 operators in 2D, 4 in 3D);
  apply/.../R4i       the stack of four interleaved in memory, a transposed view of (npoints, 4);
  fit_cloud           fit_cloud_device on the same cloud: all `no` DOFs of every point;
  gather+solve        F[hoods] gathered by torch, then ExpertSolver.solve_device on the prepared geometry (examples/time_stepping_device.py);
  csr/R1, R4          torch's own CSR product with to_sparse_csr() (the Laplacian);
  transpose           apply_transpose, one operator, one field.
Reported: medians of `alternations` rounds after a warm-up of every route, the build time of the operators, both fill values, the
bytes of the traffic model (per live entry 4 + 8 nop streamed and 8 R gathered through L2, per row 8 nop R written) with the fraction
of the 8 TB/s HBM peak that the streamed and written bytes make of each apply, and the largest distance between apply and the fit's
own DOFs contracted with the rows, in the scale sum |c_k F_k|."""
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
    ap.add_argument("--shapes", default="2-2-24,3-2-40,2-4-64", help="dimension-order-neighbours, comma separated")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.alternations >= 5, "at least 5 alternations"
    dev = torch.device("cuda", 0)
    f64 = torch.float64
    record = {"device": torch.cuda.get_device_name(0), "alternations": a.alternations, "reps_per_timing": a.reps, "npoints": a.n,
              "hbm_peak_GBps": bench.HBM_PEAK_GBPS, "method": "routes alternated in one process; HIP events; medians", "shapes": {}}
    for shape in a.shapes.split(","):
        dim, order, K = (int(v) for v in shape.split("-"))
        n, no = a.n, bench.NDOF[dim][order]
        S = torch.from_numpy(synth.halton(n, dim)).to(dev)
        S = S[bench.morton_order_device(S)].contiguous()
        F = torch.sin(3 * S[:, 0]) * torch.cos(2 * S[:, -1])
        hoods = hip.knn(S, K)
        nk = torch.full((n,), K, dtype=torch.int32, device=dev)
        knowns = torch.full((n,), 1, dtype=torch.int64, device=dev)
        wm = torch.full((n,), wlsqm.WEIGHT_CENTER, dtype=torch.int32, device=dev)
        rows = {"nop1": hip.stencil_rows(dim, order, "laplacian", device=dev), "nopG": hip.stencil_rows(dim, order, "gradient", "laplacian", device=dev)}
        ops, build_ms = {}, {}
        for name, r in rows.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            ops[name] = hip.StencilOperator(dim, order, S, hoods, nk, knowns, wm, r)
            torch.cuda.synchronize(); build_ms[name] = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize(); t0 = time.perf_counter()
        ops["nop1"].prepare_transpose()
        torch.cuda.synchronize(); build_ms["transpose"] = (time.perf_counter() - t0) * 1e3
        F4 = torch.stack([F * (1.0 + 0.25 * r) for r in range(4)])
        outs = {(name, R): torch.empty(((R,) if R > 1 else ()) + (op.nop, n), dtype=f64, device=dev) for name, op in ops.items() for R in (1, 4)}
        fi = torch.zeros((n, no), dtype=f64, device=dev)
        fi[:, 0] = F
        solver = wlsqm.ExpertSolver(dimension=dim, nk=np.full(n, K, np.int32), order=np.full(n, order, np.int32),
                                    knowns=np.full(n, 1, np.int64), weighting_method=np.full(n, wlsqm.WEIGHT_CENTER, np.int32))
        h64 = hoods.long()
        solver.prepare_device(S, S[h64].contiguous())
        fi2 = fi.clone()
        csr = ops["nop1"].to_sparse_csr(0)
        F4t = F4.t().contiguous()
        g1, gT = torch.ones((1, n), dtype=f64, device=dev), torch.empty((n,), dtype=f64, device=dev)

        routes = {"apply/%s/R%d" % (name, R): (lambda name=name, R=R: ops[name].apply(F if R == 1 else F4, out=outs[(name, R)]))
                  for name in ops for R in (1, 4)}
        # the four fields interleaved, (npoints, 4) in memory: one gather touches one 32-byte piece instead of four lines
        routes["apply/nop1/R4i"] = lambda: ops["nop1"].apply(F4t.t(), out=outs[("nop1", 4)])
        routes["apply/nopG/R4i"] = lambda: ops["nopG"].apply(F4t.t(), out=outs[("nopG", 4)])
        routes["fit_cloud"] = lambda: hip.fit_cloud_device(dim, order, S, F, hoods, fi, nk, knowns, wm)
        routes["gather+solve"] = lambda: solver.solve_device(F[h64], fi2)
        routes["csr/R1"] = lambda: torch.mv(csr, F)
        routes["csr/R4"] = lambda: torch.sparse.mm(csr, F4t)
        routes["transpose"] = lambda: ops["nop1"].apply_transpose(g1, out=gT)
        for fn in routes.values():                                    # warm-up of every route
            fn()
        torch.cuda.synchronize()
        # the routes give the same numbers: apply against the fit's DOFs contracted with the rows, in the scale sum |c_k F_k|
        slots, own = ops["nopG"].coefficients()
        scale = (slots.abs() * F[h64].abs()[None]).sum(dim=2) + own.abs() * F.abs()[None]
        agree = float(((outs[("nopG", 1)] - torch.einsum("oa,ja->oj", rows["nopG"], fi)).abs() / scale.clamp_min(1e-300)).max())
        agree_csr = float(((torch.mv(csr, F) - outs[("nop1", 1)][0]).abs() / ((ops["nop1"].coefficients()[0][0].abs() * F[h64].abs()).sum(dim=1)
                                                                             + ops["nop1"].coefficients()[1][0].abs() * F.abs()).clamp_min(1e-300)).max())
        del slots, own, scale
        ms = {k: [] for k in routes}
        for _ in range(a.alternations):
            for k, fn in routes.items():
                ms[k].append(events(fn, a.reps))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        nnz = n * (K + 1)
        model = {}
        for name, op in ops.items():
            for R in (1, 4):
                streamed = nnz * (4 + 8 * op.nop) + n * 8 * op.nop * R
                model["apply/%s/R%d" % (name, R)] = {
                    "bytes_streamed_and_written": streamed, "bytes_gathered_through_L2": nnz * 8 * R,
                    "hbm_frac": streamed / (med["apply/%s/R%d" % (name, R)] * 1e-3) / (bench.HBM_PEAK_GBPS * 1e9)}
        rec = {"dimension": dim, "order": order, "nk": K, "no": no, "npoints": n, "nop": {k: op.nop for k, op in ops.items()},
               "median_ms": med, "ms_all": {k: [round(v, 5) for v in ms[k]] for k in ms}, "build_ms": build_ms,
               "fill": ops["nop1"].fill, "fill_transposed": ops["nop1"].fill_transposed,
               "memory_used_bytes": {k: op.memory_used() for k, op in ops.items()}, "traffic_model": model,
               "largest_distance_apply_to_fit_cloud": agree, "largest_distance_apply_to_csr": agree_csr}
        record["shapes"][shape] = rec
        print("%s n=%d | " % (shape, n) + "  ".join("%s %.4f" % (k, v) for k, v in med.items()) + " ms | build %s ms | fill %.3f / %.3f | "
              "apply nop1 R1 %.3f of peak | vs fit %.1e vs csr %.1e"
              % ({k: round(v, 1) for k, v in build_ms.items()}, rec["fill"], rec["fill_transposed"], model["apply/nop1/R1"]["hbm_frac"], agree, agree_csr),
              flush=True)
        for op in ops.values():
            op.close()
        solver.close()
        del routes, outs, ops, csr, solver, S, F, F4, F4t, hoods, h64, fi, fi2
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
