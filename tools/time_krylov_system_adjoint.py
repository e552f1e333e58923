#!/usr/bin/env python
"""The gradients through coupled solves (wlsqm.hip.differentiable_stencil_system_solve), timed on one GPU in one
process, the routes ALTERNATED (the method of tools/time_krylov.py):
    python tools/time_krylov_system_adjoint.py [--shapes 2-24,3-40] [--n 1000000] [--alternations 7] [--out profiles/krylov_system_adjoint_timings.json]
Clouds and planes: the two elasticity clouds of tools/time_krylov_system.py (n Halton points in Morton order, K nearest neighbours,
order 2; the second-derivative planes with zero rows on the 1.2 h band and one `value` plane; m = dimension, nop = 4 or 7).
  1. StencilSystemSolver.gradients ("krylov-system-grads": one pass for values and diag, into buffers allocated beforehand) against the
     same quantities from torch index operations on the operator's arrays — the route a user has without the kernel, its index arrays
     prepared outside the timed region — asserted to agree to 1e-12 of the largest entry; values alone and diag alone as well, and
     each kernel route again as 10 and 20 calls back to back (ms per call = the difference over 10: without the host's share);
     coupling_gradient (the stacked product and a contraction, no kernel of its own) is timed beside them.
     The traffic model, bytes per point with all outputs, counted from the kernel: (4 + 8 nop)(K + 1) for col and the planes written,
     4 for len, 16 m for the point's lam and x, 8 m^2 for diag; the gathered neighbour values are not counted (cache hits on a cloud in
     Morton order), as section 24 counts its product.
  2. forward and backward of differentiable_stencil_system_solve, HIP events around one call each (host reads of the solves' scalars
     included), with gradients wanted by b alone, by b and coupling, by b and the point table S, and the iteration counts.  The system
     of this part is the implicit step (I + 0.25 h^2 E) x = b, E the elasticity operator (lambda = mu = 1) of the planes: the stationary
     problem E x = b at 1M points is beyond a solver whose only preconditioner is the scalar diagonal, and a timed solve must converge.
Medians of `alternations` rounds after a warm-up of every route.  Records, no thresholds."""
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
from time_krylov_system import SECOND, elasticity_coupling, events  # noqa: E402


def cloud(dim, K, n, dev):
    """(S, operator) of tools/time_krylov_system.py's elasticity cloud."""
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
    return S, hip.StencilOperator(dim, 2, S, hoods, nk, knowns, wm, rows)


def time_gradients(op, dim, K, n, alternations):
    dev, f64 = op._device, torch.float64
    m, nop, total = dim, op.nop, op._m["total"]
    cp = elasticity_coupling(dim)
    solver = hip.StencilSystemSolver(op, cp, diag=0.0)
    gen = torch.Generator(device=dev).manual_seed(3)
    lam, x = (torch.randn((n, m), dtype=f64, device=dev, generator=gen) for _ in range(2))
    outs = (torch.empty((nop, total), dtype=f64, device=dev), torch.empty((m, m, n), dtype=f64, device=dev))
    src, row = op._entries()
    col = op._m["col"][src].long()
    cpt = torch.from_numpy(cp).to(dev)
    t_values = torch.zeros((nop, total), dtype=f64, device=dev)
    t_diag = torch.empty((m, m, n), dtype=f64, device=dev)

    def torch_values():
        # plane by plane through 1-D index operations, the form in which torch's gather and scatter are fastest (one 2-D
        # `t_values[:, src] = ...` of all planes took 51 ms in 2D and 73 ms in 3D)
        u = torch.einsum("abo,ja->obj", cpt, lam)                         # (nop, m, n)
        xc = x[col].t()                                                   # (m, entries)
        for o in range(nop):
            t_values[o][src] = -(u[o][:, row] * xc).sum(dim=0)

    def torch_diag():
        torch.mul(lam.t()[:, None, :], x.t()[None, :, :], out=t_diag).neg_()

    def torch_all():
        torch_values(); torch_diag()

    routes = {"kernel_all": lambda: solver.gradients(lam, x, values=outs[0], diag=outs[1]), "torch_all": torch_all,
              "kernel_values": lambda: solver.gradients(lam, x, values=outs[0]), "torch_values": torch_values,
              "kernel_diag": lambda: solver.gradients(lam, x, diag=outs[1]), "torch_diag": torch_diag,
              "coupling_gradient": lambda: solver.coupling_gradient(lam, x)}
    for fn in routes.values():
        fn()
    agree = {"values": float((t_values - outs[0]).abs().max() / outs[0].abs().max()),
             "diag": float((t_diag - outs[1]).abs().max() / outs[1].abs().max())}
    assert max(agree.values()) <= 1e-12, "the kernel and the torch route differ by %r of the largest entry" % (agree,)

    def back_to_back(fn):
        """ms per call from 10 and 20 calls enqueued back to back: the time of the launches themselves once the device is busy, where
        the events around ONE call also hold the host's argument checks in front of an idle device."""
        t10, t20 = (events(lambda: [fn() for _ in range(N)]) for N in (10, 20))
        return (t20 - t10) / 10.0

    ms = {k: [] for k in routes}
    steady = {k: [] for k in routes if k.startswith("kernel_")}
    for _ in range(alternations):
        for k, fn in routes.items():
            ms[k].append(events(fn))
        for k in steady:
            steady[k].append(back_to_back(routes[k]))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    smed = {k: float(np.median(v)) for k, v in steady.items()}
    per_point = {"all": (4 + 8 * nop) * (K + 1) + 4 + 16 * m + 8 * m * m, "values": (4 + 8 * nop) * (K + 1) + 4 + 8 * m,
                 "diag": 16 * m + 8 * m * m}
    frac = {k: per_point[k] * n / (med["kernel_" + k] * 1e-3) / (bench.HBM_PEAK_GBPS * 1e9) for k in per_point}
    sfrac = {k: per_point[k] * n / (smed["kernel_" + k] * 1e-3) / (bench.HBM_PEAK_GBPS * 1e9) for k in per_point}
    solver.close()
    return {"stored_entries_per_point": total / n, "gradients_median_ms": med,
            "gradients_ms_all": {k: [round(v, 5) for v in vs] for k, vs in ms.items()},
            "ratio_torch_over_kernel": {k: med["torch_" + k] / med["kernel_" + k] for k in per_point},
            "back_to_back_ms_per_call": smed, "back_to_back_ms_all": {k: [round(v, 5) for v in vs] for k, vs in steady.items()},
            "model_bytes_per_point": per_point, "hbm_frac_by_model": frac, "hbm_frac_by_model_back_to_back": sfrac,
            "torch_against_kernel": agree}


def time_autograd(op, S, dim, n, alternations):
    dev, f64 = op._device, torch.float64
    m = dim
    tau = 0.25 * n ** (-2.0 / dim)
    cp = torch.from_numpy(tau * elasticity_coupling(dim))
    solver = hip.StencilSystemSolver(op, cp.numpy(), diag=1.0)
    solver.prepare_transpose()
    b0 = torch.stack([torch.sin((3 + a) * S[:, 0]) * torch.cos((2 + a) * S[:, -1]) for a in range(m)], dim=1).contiguous()
    w = torch.stack([torch.cos((5 + a) * S[:, 0]) + S[:, -1] for a in range(m)], dim=1).contiguous()
    iters = {}

    def timed(kind):
        loss = [None]

        def fwd():
            b = b0.clone().requires_grad_()
            kw = {}
            if kind == "b_coupling":
                kw["coupling"] = cp.clone().requires_grad_()
            if kind == "b_S":
                kw["S"] = S.clone().requires_grad_()
            loss[0] = (hip.differentiable_stencil_system_solve(solver, b, maxiter=400, **kw) * w).sum()
        t_f = events(fwd)
        iters.setdefault(kind, {})["forward"] = solver.info().iterations
        t_b = events(lambda: loss[0].backward())
        iters[kind]["adjoint"] = solver.info().iterations
        return t_f, t_b

    kinds = ("b", "b_coupling", "b_S")
    for k in kinds:
        timed(k)
    ms = {k: {"forward": [], "backward": []} for k in kinds}
    for _ in range(alternations):
        for k in kinds:
            t_f, t_b = timed(k)
            ms[k]["forward"].append(t_f); ms[k]["backward"].append(t_b)
    med = {k: {p: float(np.median(v)) for p, v in ms[k].items()} for k in kinds}
    solver.close()
    return {"system": "(I + 0.25 h^2 E) x = b, Jacobi, rtol 1e-10, loss = w . x", "iterations": iters, "median_ms": med,
            "backward_over_forward": {k: med[k]["backward"] / med[k]["forward"] for k in kinds},
            "ms_all": {k: {p: [round(v, 5) for v in vs] for p, vs in ms[k].items()} for k in ms}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2-24,3-40", help="dimension-neighbours, comma separated")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.alternations >= 5, "at least 5 alternations"
    dev = torch.device("cuda", 0)
    record = {"device": torch.cuda.get_device_name(0), "alternations": a.alternations, "npoints": a.n,
              "method": "routes alternated in one process; HIP events around one call each; medians",
              "baseline": "the same gradients from torch index operations on the operator's arrays, index arrays prepared beforehand",
              "model": "bytes per point, all outputs: (4 + 8 nop)(K + 1) + 4 + 16 m + 8 m^2", "clouds": {}}
    for shape in a.shapes.split(","):
        dim, K = (int(v) for v in shape.split("-"))
        S, op = cloud(dim, K, a.n, dev)
        rec = dict(dimension=dim, order=2, nk=K, npoints=a.n, m=dim, nop=op.nop, **time_gradients(op, dim, K, a.n, a.alternations))
        rec["autograd"] = time_autograd(op, S, dim, a.n, a.alternations)
        name = "%s n=%d" % (shape, a.n)
        record["clouds"][name] = rec
        g, au = rec["gradients_median_ms"], rec["autograd"]
        print("%s | gradients ms  kernel %.4f torch %.4f (x%.1f), values %.4f / %.4f, diag %.4f / %.4f, coupling %.4f | model %d B/point, %.3f of "
              "peak (values %.3f) | agree %.1e %.1e" % (name, g["kernel_all"], g["torch_all"], rec["ratio_torch_over_kernel"]["all"],
              g["kernel_values"], g["torch_values"], g["kernel_diag"], g["torch_diag"], g["coupling_gradient"],
              rec["model_bytes_per_point"]["all"], rec["hbm_frac_by_model"]["all"], rec["hbm_frac_by_model"]["values"],
              rec["torch_against_kernel"]["values"], rec["torch_against_kernel"]["diag"]), flush=True)
        print("  back to back, ms per call: all %.4f (%.3f of peak), values %.4f, diag %.4f" % (
            rec["back_to_back_ms_per_call"]["kernel_all"], rec["hbm_frac_by_model_back_to_back"]["all"],
            rec["back_to_back_ms_per_call"]["kernel_values"], rec["back_to_back_ms_per_call"]["kernel_diag"]), flush=True)
        print("  forward / backward ms  " + "  ".join("%s %.2f / %.2f (%d / %d iterations)" % (
            k, au["median_ms"][k]["forward"], au["median_ms"][k]["backward"], au["iterations"][k]["forward"], au["iterations"][k]["adjoint"])
            for k in au["median_ms"]), flush=True)
        op.close()
        del S, op
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
