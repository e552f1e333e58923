#!/usr/bin/env python
"""StencilOperator.update against the other routes to the same coefficients, ALTERNATED in one process on one GPU, as tools/time_stencil.py:
    python tools/time_stencil_update.py [--shapes 2-2-24,3-2-40,2-4-64] [--n 1000000] [--alternations 7] [--out profiles/stencil_update_timings.json]
Clouds: n Halton points in Morton order, the K nearest neighbours of each, the function value known (b_F), centre weighting.  Routes, HIP
events around REPS back-to-back calls, for one operator (the Laplacian, nop1) and for the gradient and the Laplacian (nopG):
  update/...          (a) op.update(S, check=False): the fused kernel "stencil-build";
  update+hoods/...        the same with hoods= (the columns rewritten too);
  constructor/...     (b) StencilOperator(...) on the same arguments: nop adjoint launches, scatter, pack (it synchronises);
  adjoint/...         (c) nop calls of fit_cloud_adjoint_device with every output preallocated;
  fit_cloud           (d) one fit_cloud_device;
  update+T/nop1       (e) update on an operator whose transposed matrix is built: the permute kernel rides along; its cost is the
                          difference to update/nop1;
  apply/...               op.apply(F, out=), for the break-even count.
Reported: medians of `alternations` rounds after a warm-up of every route; (b) / (a); the break-even count m, the smallest number of
applies per update at which update + m applies is cheaper than m fit_cloud_device calls; the bytes of the traffic model (per live entry 4
of index read and 8 nop of values written, 4 more with hoods=; per case 8 nop no of known_coef; the points are gathered through L2 three
times, 3 * 8 * dim per entry) with the fraction of the 8 TB/s HBM peak that the streamed bytes make of each update."""
import argparse
import json
import math
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
        geo = (S, hoods, nk, knowns, wm)
        rows = {"nop1": hip.stencil_rows(dim, order, "laplacian", device=dev), "nopG": hip.stencil_rows(dim, order, "gradient", "laplacian", device=dev)}
        ops = {name: hip.StencilOperator(dim, order, *geo, r) for name, r in rows.items()}
        opT = hip.StencilOperator(dim, order, *geo, rows["nop1"])
        opT.prepare_transpose()
        # the points where they are a step later: moved by a thousandth of the spacing, the neighbour lists kept
        S2 = (S + 1e-3 * n ** (-1.0 / dim) * torch.sin(7 * S.flip(-1))).contiguous()
        outs = {name: torch.empty((op.nop, n), dtype=f64, device=dev) for name, op in ops.items()}
        fi = torch.zeros((n, no), dtype=f64, device=dev)
        fi[:, 0] = F
        g = {name: [r[o].expand(n, no).contiguous() for o in range(r.shape[0])] for name, r in rows.items()}
        slots, gfi, gF = torch.empty((n, K), dtype=f64, device=dev), torch.empty((n, no), dtype=f64, device=dev), torch.empty((n,), dtype=f64, device=dev)

        def adjoints(name):
            for go in g[name]:
                hip.fit_cloud_adjoint_device(dim, order, S2, hoods, nk, knowns, wm, go, grad_F=gF, grad_fi=gfi, slots=slots)

        routes = {}
        for name in ops:
            routes["update/" + name] = lambda name=name: ops[name].update(S2, check=False)
            routes["update+hoods/" + name] = lambda name=name: ops[name].update(S2, hoods=hoods, check=False)
            routes["constructor/" + name] = lambda name=name: hip.StencilOperator(dim, order, S2, hoods, nk, knowns, wm, rows[name]).close()
            routes["adjoint/" + name] = lambda name=name: adjoints(name)
            routes["apply/" + name] = lambda name=name: ops[name].apply(F, out=outs[name])
        routes["fit_cloud"] = lambda: hip.fit_cloud_device(dim, order, S2, F, hoods, fi, nk, knowns, wm)
        routes["update+T/nop1"] = lambda: opT.update(S2, check=False)
        for fn in routes.values():                                    # warm-up of every route
            fn()
        torch.cuda.synchronize()
        # the routes give the same coefficients: update against the constructor on the moved cloud, in units of the largest coefficient
        want = hip.StencilOperator(dim, order, S2, hoods, nk, knowns, wm, rows["nopG"])
        ops["nopG"].update(S2, check=False)
        agree = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(ops["nopG"].coefficients(), want.coefficients()))
        same_bits = all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(ops["nopG"].coefficients(), want.coefficients()))
        want.close()
        ms = {k: [] for k in routes}
        for _ in range(a.alternations):
            for k, fn in routes.items():
                ms[k].append(events(fn, a.reps))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        nnz = n * (K + 1)
        model, derived = {}, {}
        for name, op in ops.items():
            for route, col in (("update/", 0), ("update+hoods/", 4)):
                streamed = nnz * (4 + col + 8 * op.nop) + n * 8 * op.nop * no
                model[route + name] = {"bytes_streamed": streamed, "bytes_gathered_through_L2": 3 * nnz * 8 * dim,
                                       "hbm_frac": streamed / (med[route + name] * 1e-3) / (bench.HBM_PEAK_GBPS * 1e9)}
            gain = med["fit_cloud"] - med["apply/" + name]
            derived[name] = {"constructor_over_update": med["constructor/" + name] / med["update/" + name],
                             "adjoint_over_update": med["adjoint/" + name] / med["update/" + name],
                             "break_even_applies_per_update": math.floor(med["update/" + name] / gain) + 1 if gain > 0 else None}
        derived["update_nopG_over_nop1"] = med["update/nopG"] / med["update/nop1"]
        derived["transposed_refresh_ms"] = med["update+T/nop1"] - med["update/nop1"]
        rec = {"dimension": dim, "order": order, "nk": K, "no": no, "npoints": n, "nop": {k: op.nop for k, op in ops.items()},
               "median_ms": med, "ms_all": {k: [round(v, 5) for v in ms[k]] for k in ms}, "derived": derived, "traffic_model": model,
               "largest_distance_update_to_constructor": agree, "update_is_the_constructors_bits": same_bits}
        record["shapes"][shape] = rec
        print("%s n=%d | " % (shape, n) + "  ".join("%s %.4f" % (k, v) for k, v in med.items()) + " ms | " + json.dumps(derived)
              + " | update nop1 %.3f of peak | vs constructor %.1e (bits: %s)" % (model["update/nop1"]["hbm_frac"], agree, same_bits), flush=True)
        for op in list(ops.values()) + [opT]:
            op.close()
        del routes, outs, ops, opT, S, S2, F, hoods, fi, g, slots, gfi, gF
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
