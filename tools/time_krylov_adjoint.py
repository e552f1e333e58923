#!/usr/bin/env python
"""The gradients through implicit solves (wlsqm.hip.differentiable_stencil_solve), timed on one GPU in one process,
the routes ALTERNATED (the method of tools/time_krylov.py):
    python tools/time_krylov_adjoint.py [--shapes 2-2-24,3-2-40,2-4-64] [--n 1000000] [--alternations 7] [--out profiles/krylov_adjoint_timings.json]
Clouds and system: those of tools/time_krylov.py, (I - 0.25 h^2 Lap_h) x = b, Jacobi, rtol 1e-10, loss = (w . x).
  1. forward and backward of differentiable_stencil_solve, HIP events around one call each (they include the host reads of the solves'
     scalars, as a user pays them), with gradients wanted by b alone, by b and a diag tensor, by b and the point table S;
  2. StencilSolver.gradients (one pass of "krylov-grads" for values, diag and scale) against the same quantities from torch index
     operations on the operator's arrays, both into buffers allocated beforehand where torch allows it.
Medians of `alternations` rounds after a warm-up of every route.  Records, no thresholds."""
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


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2-2-24,3-2-40,2-4-64", help="dimension-order-neighbours, comma separated")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.alternations >= 5, "at least 5 alternations"
    dev = torch.device("cuda", 0)
    f64 = torch.float64
    record = {"device": torch.cuda.get_device_name(0), "alternations": a.alternations, "npoints": a.n,
              "system": "I - 0.25 h^2 Laplacian, Jacobi, rtol 1e-10, loss = w . x",
              "method": "routes alternated in one process; HIP events around one call each (host reads of the solves included); medians",
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
        op = hip.StencilOperator(dim, order, S, hoods, nk, knowns, wm, hip.stencil_rows(dim, order, "laplacian", device=dev))
        op.prepare_transpose()
        scale = -0.25 * n ** (-2.0 / dim)
        b0 = torch.sin(3 * S[:, 0]) * torch.cos(2 * S[:, -1])
        w = torch.cos(5 * S[:, 0]) + S[:, -1]
        plain = hip.StencilSolver(op, diag=1.0, scale=scale)
        diag = torch.ones(n, dtype=f64, device=dev).requires_grad_()
        with_diag = hip.StencilSolver(op, diag=diag, scale=scale)
        iters = {}

        def forward(kind):
            b = b0.clone().requires_grad_()
            if kind == "b_S":
                x = hip.differentiable_stencil_solve(plain, b, S=S.clone().requires_grad_(), maxiter=200)
            else:
                x = hip.differentiable_stencil_solve(with_diag if kind == "b_diag" else plain, b, maxiter=200)
            return (x * w).sum()

        def timed(kind):
            loss = [None]

            def fwd():
                loss[0] = forward(kind)
            t_f = events(fwd)
            solver = with_diag if kind == "b_diag" else plain
            iters.setdefault(kind, {})["forward"] = solver.info().iterations
            t_b = events(lambda: loss[0].backward())
            iters[kind]["adjoint"] = solver.info().iterations
            diag.grad = None
            return t_f, t_b

        kinds = ("b", "b_diag", "b_S")
        for k in kinds:
            timed(k)
        ms = {k: {"forward": [], "backward": []} for k in kinds}
        for _ in range(a.alternations):
            for k in kinds:
                t_f, t_b = timed(k)
                ms[k]["forward"].append(t_f); ms[k]["backward"].append(t_b)
        med = {k: {p: float(np.median(v)) for p, v in ms[k].items()} for k in kinds}

        # 2. the grads kernel against torch index operations
        x = torch.zeros(n, dtype=f64, device=dev)
        lam = torch.zeros(n, dtype=f64, device=dev)
        assert plain.solve(b0, x, maxiter=200).status == 0 and plain.solve(w, lam, maxiter=200, transpose=True).status == 0
        total = op._m["total"]
        src, row = op._entries()
        col = op._m["col"][src].long()
        outs = (torch.empty(total, dtype=f64, device=dev), torch.empty(n, dtype=f64, device=dev), torch.empty((), dtype=f64, device=dev))
        t_values = torch.zeros(total, dtype=f64, device=dev)
        t_diag = torch.empty(n, dtype=f64, device=dev)
        t_apply = torch.empty((1, n), dtype=f64, device=dev)

        def kernel_all():
            plain.gradients(lam, x, values=outs[0], diag=outs[1], scale=outs[2])

        def kernel_values():
            plain.gradients(lam, x, values=outs[0])

        def torch_all():
            t_values[src] = -((scale * lam[row]) * x[col])
            torch.mul(lam, x, out=t_diag).neg_()
            op.apply(x, out=t_apply)
            return -torch.dot(lam, t_apply[0])

        def torch_values():
            t_values[src] = -((scale * lam[row]) * x[col])

        routes = {"kernel_all": kernel_all, "torch_all": torch_all, "kernel_values": kernel_values, "torch_values": torch_values}
        for fn in routes.values():
            fn()
        agree = {"values": float((t_values - outs[0]).abs().max()), "diag": float((t_diag - outs[1]).abs().max()),
                 "scale_relative": float(((torch_all() - outs[2]) / outs[2]).abs())}
        gms = {k: [] for k in routes}
        for _ in range(a.alternations):
            for k, fn in routes.items():
                gms[k].append(events(fn))
        gmed = {k: float(np.median(v)) for k, v in gms.items()}
        model = total * (4 + 8 + 8) + n * (4 * 8 + 4)
        rec = {"dimension": dim, "order": order, "nk": K, "npoints": n, "stored_entries": total, "iterations": iters,
               "median_ms": med, "backward_over_forward": {k: med[k]["backward"] / med[k]["forward"] for k in kinds},
               "ms_all": {k: {p: [round(v, 5) for v in vs] for p, vs in ms[k].items()} for k in ms},
               "gradients_median_ms": gmed, "gradients_ms_all": {k: [round(v, 5) for v in vs] for k, vs in gms.items()},
               "ratio_torch_over_kernel": {"all": gmed["torch_all"] / gmed["kernel_all"], "values": gmed["torch_values"] / gmed["kernel_values"]},
               "gradients_traffic_model_bytes": model,
               "gradients_hbm_frac": model / (gmed["kernel_all"] * 1e-3) / (bench.HBM_PEAK_GBPS * 1e9),
               "torch_against_kernel": agree}
        record["shapes"][shape] = rec
        print("%s n=%d | forward / backward ms  b %.2f / %.2f  b+diag %.2f / %.2f  b+S %.2f / %.2f | gradients ms  kernel %.4f torch %.4f (x%.1f), "
              "values alone %.4f / %.4f | model %.0f MB, %.3f of peak | agree %.1e %.1e %.1e"
              % (shape, n, med["b"]["forward"], med["b"]["backward"], med["b_diag"]["forward"], med["b_diag"]["backward"], med["b_S"]["forward"],
                 med["b_S"]["backward"], gmed["kernel_all"], gmed["torch_all"], rec["ratio_torch_over_kernel"]["all"], gmed["kernel_values"],
                 gmed["torch_values"], model / 1e6, rec["gradients_hbm_frac"], agree["values"], agree["diag"], agree["scale_relative"]), flush=True)
        plain.close(); with_diag.close(); op.close()
        del routes, outs, t_values, t_diag, t_apply, src, row, col, S, hoods, x, lam, diag
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
