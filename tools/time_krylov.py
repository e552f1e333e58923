#!/usr/bin/env python
"""The device-resident BiCGSTAB of wlsqm.hip.StencilSolver against the same recurrence in torch operations, ALTERNATED in one process on
one GPU (the method of tools/time_stencil.py: a ratio is only good inside one process):
    python tools/time_krylov.py [--shapes 2-2-24,3-2-40,2-4-64] [--n 1000000] [--alternations 7] [--out profiles/krylov_timings.json]
Clouds: those of tools/time_stencil.py (n Halton points in Morton order, K nearest neighbours, b_F known, centre weighting).  System:
(I - 0.25 h^2 Lap_h) x = b, h = n^(-1/dim), Jacobi, rtol = atol = 0 so that no solve stops before its iteration limit (checked: a timed run that
does not end with status 1 at exactly the iterations asked for is listed under stopped_early).  Routes, HIP events around one call each:
  (a) eager    solver.enqueue(b, x, N);
  (b) graph    the same captured once and replayed;
  (c) torch    the same recurrence in torch operations around op.apply, what a user can write without the solver — in its most favourable
               form: every scalar stays a 0-d device tensor, so that there is no host read at all, and nothing allocates vectors.
Each route runs with N = 10 and N = 20 iterations; ms per iteration is the difference over 10 (the start of a solve — the diagonal, the first
residual — drops out; it is reported on its own as start_ms).  Medians of `alternations` rounds after a warm-up of every route.
The traffic model of DESIGN.md section 17, per iteration: 2 passes over 4 + 8 bytes per stored entry, 25 vector reads and writes of 8
bytes and 2 of 4 (len) per point; its fraction of the 8 TB/s HBM peak at route (a)'s and (b)'s time is reported."""
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


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


class TorchBiCGSTAB:
    """Route (c): the recurrence of csrc/krylov.hip in torch operations; all buffers allocated here, scalars as 0-d device tensors."""

    def __init__(self, op, scale, n, device):
        z = lambda: torch.empty(n, dtype=torch.float64, device=device)
        self.op, self.scale = op, scale
        self.r, self.r0, self.p, self.v, self.s, self.t, self.ph, self.sh, self.dinv, self.tmp = (z() for _ in range(10))
        self.out = torch.empty((1, n), dtype=torch.float64, device=device)

    def product(self, x, y):            # y = x + scale A x
        self.op.apply(x, out=self.out, alpha=self.scale)
        torch.add(x, self.out[0], out=y)

    def run(self, b, x, iterations, dinv):
        r, r0, p, v, s, t, ph, sh, tmp = self.r, self.r0, self.p, self.v, self.s, self.t, self.ph, self.sh, self.tmp
        self.product(x, tmp)
        torch.sub(b, tmp, out=r)
        r0.copy_(r)
        rho = torch.dot(r0, r)
        rho_old = alpha = omega = None
        for it in range(iterations):
            if it == 0:
                p.copy_(r)
            else:
                beta = (rho / rho_old) * (alpha / omega)
                torch.addcmul(p, omega, v, value=-1.0, out=tmp)          # p - omega v
                torch.addcmul(r, beta, tmp, out=p)
            torch.mul(dinv, p, out=ph)
            self.product(ph, v)
            alpha = rho / torch.dot(r0, v)
            torch.addcmul(r, alpha, v, value=-1.0, out=s)
            torch.mul(dinv, s, out=sh)
            self.product(sh, t)
            omega = torch.dot(t, s) / torch.dot(t, t)
            x.addcmul_(alpha, ph).addcmul_(omega, sh)
            torch.addcmul(s, omega, t, value=-1.0, out=r)
            rho_old, rho = rho, torch.dot(r0, r)
        return torch.dot(r, r)


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
    record = {"device": torch.cuda.get_device_name(0), "alternations": a.alternations, "npoints": a.n, "iterations": [N1, N2],
              "hbm_peak_GBps": bench.HBM_PEAK_GBPS, "system": "I - 0.25 h^2 Laplacian, Jacobi, no stop before the iteration limit",
              "method": "routes alternated in one process; HIP events; medians; ms per iteration = (ms of 20 - ms of 10) / 10", "shapes": {}}
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
        scale = -0.25 * n ** (-2.0 / dim)
        solver = hip.StencilSolver(op, diag=1.0, scale=scale)
        b = torch.sin(3 * S[:, 0]) * torch.cos(2 * S[:, -1])
        xs = {k: torch.zeros(n, dtype=f64, device=dev) for k in ("a", "b", "c")}
        # a converging solve first: what the timed iterations are iterations of
        info = solver.solve(b, xs["a"], rtol=1e-10, maxiter=200)
        res = torch.empty(n, dtype=f64, device=dev)
        res, _, rr = solver.product(xs["a"], out=res)
        true = float((b - res).norm() / b.norm())
        tc = TorchBiCGSTAB(op, scale, n, dev)
        slots, own = op.coefficients()
        dinv = 1.0 / (1.0 + scale * (own[0] + (slots[0] * (hoods.long() == torch.arange(n, device=dev)[:, None])).sum(dim=1)))
        del slots, own
        graphs = {}
        for N in (N1, N2):
            xs["b"].zero_()
            solver.enqueue(b, xs["b"], N, rtol=0.0)                      # warm-up outside the capture
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=torch.cuda.Stream()):
                solver.enqueue(b, xs["b"], N, rtol=0.0)
            graphs[N] = g
        torch.cuda.synchronize()

        def route_a(N):
            xs["a"].zero_()
            return events(lambda: solver.enqueue(b, xs["a"], N, rtol=0.0))

        def route_b(N):
            xs["b"].zero_()
            return events(graphs[N].replay)

        def route_c(N):
            xs["c"].zero_()
            return events(lambda: tc.run(b, xs["c"], N, dinv))

        routes = {"a_eager": route_a, "b_graph": route_b, "c_torch": route_c}
        for fn in routes.values():                                    # warm-up of every route
            fn(N1); fn(N2)
        # the routes compute the same solve: after N2 iterations from zero, against each other in the scale of the solution
        agree = {k: float((xs[k] - xs["a"]).norm() / xs["a"].norm()) for k in ("b", "c")}
        ms = {k: {N1: [], N2: []} for k in routes}
        early = []                                                    # timed solves that stopped before their limit: their times do not count
        for _ in range(a.alternations):
            for k, fn in routes.items():
                for N in (N1, N2):
                    ms[k][N].append(fn(N))
                    if k != "c_torch":
                        got = solver.info()
                        if (got.status, got.iterations) != (1, N):
                            early.append((k, N, got.status, got.iterations))
        med = {k: {N: float(np.median(v)) for N, v in ms[k].items()} for k in routes}
        per_it = {k: (med[k][N2] - med[k][N1]) / (N2 - N1) for k in routes}
        start = {k: med[k][N1] - N1 * per_it[k] for k in routes}
        total = op._m["total"]
        model = 2 * total * (4 + 8) + n * (25 * 8 + 2 * 4)
        rec = {"dimension": dim, "order": order, "nk": K, "npoints": n, "fill": op.fill, "stored_entries": total,
               "ms_per_iteration": per_it, "start_ms": start, "median_ms": {k: {str(N): v for N, v in med[k].items()} for k in med},
               "ms_all": {k: {str(N): [round(v, 5) for v in vs] for N, vs in ms[k].items()} for k in ms},
               "ratio_torch_over_eager": per_it["c_torch"] / per_it["a_eager"], "ratio_torch_over_graph": per_it["c_torch"] / per_it["b_graph"],
               "traffic_model_bytes_per_iteration": model,
               "hbm_frac": {k: model / (per_it[k] * 1e-3) / (bench.HBM_PEAK_GBPS * 1e9) for k in ("a_eager", "b_graph")},
               "converging_solve": {"status": info.status, "iterations": info.iterations, "recursive_residual_over_b": info.residual / float(b.norm()),
                                    "true_residual_over_b": true},
               "distance_to_eager_after_%d_iterations" % N2: agree, "stopped_early": early, "memory_used_bytes": {"operator": op.memory_used(), "solver": solver.memory_used()}}
        record["shapes"][shape] = rec
        print("%s n=%d | ms/iteration  eager %.4f  graph %.4f  torch %.4f | torch/eager %.2f torch/graph %.2f | model %.0f MB, %.3f / %.3f of peak | "
              "start %.3f ms | solve: %d iterations, true residual %.2e | agree %.1e %.1e"
              % (shape, n, per_it["a_eager"], per_it["b_graph"], per_it["c_torch"], rec["ratio_torch_over_eager"], rec["ratio_torch_over_graph"],
                 model / 1e6, rec["hbm_frac"]["a_eager"], rec["hbm_frac"]["b_graph"], start["a_eager"], info.iterations, true, agree["b"], agree["c"]),
              flush=True)
        if early:
            print("  NOT VALID: solves stopped before their iteration limit: %s" % early[:4], flush=True)
        solver.close(); op.close()
        del routes, graphs, tc, xs, S, hoods, b, res, dinv
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
