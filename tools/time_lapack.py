"""Per-instance device time of the batched dense solves (wlsqm.hip.*_batched, the kernels behind wlsqm.utils.lapackdrivers).

usage: python tools/time_lapack.py [--out profiles/lapack_timings.json] [--sizes 2,3,6] [--quick]

Device-resident inputs, HIP-event timing on the current stream, median of 5 launches (the matrices are restored from a
pristine copy before every launch, outside the timed interval).  The batch of each size is grown until one launch takes
>= 100 us (memory permitting).  Every line carries the algorithmic bytes and fp64 flops per system, counted from the
shapes, and the fraction of the bounding roof (8 TB/s HBM, 78.6 TF/s fp64 vector).  Also measured: numpy's stacked
np.linalg.solve on this host (the CPU baseline) and the host-array path of wlsqm.utils.lapackdrivers.mgeneral at n = 6
with 10^6 systems, which moves every byte over PCIe and is bound by it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-wlsqm_amd"))

import torch  # noqa: E402

from wlsqm import hip as H  # noqa: E402
from wlsqm.utils import lapackdrivers as L  # noqa: E402

HBM = 8.0e12
FP64 = 78.6e12
SIZES = [2, 3, 4, 6, 10, 15, 20, 35, 60, 100, 300]
MEM_CAP = 2.0e9            # bytes of matrices per batch


def model(family, n):
    """(bytes, flops) per system"""
    A, vec, piv = 8 * n * n, 8 * n, 4 * n
    lu, bk, sol = 2.0 * n ** 3 / 3, n ** 3 / 3.0, 2.0 * n * n
    if family == "gesv":
        return 2 * A + 2 * vec + piv + 4, lu + sol
    if family == "getrf+getrs":
        return (2 * A + piv + 4) + (A + piv + 2 * vec), lu + sol
    if family == "sysv":
        return 2 * A + 2 * vec + piv + 4, bk + sol
    if family == "sytrf+sytrs":
        return (2 * A + piv + 4) + (A + piv + 2 * vec), bk + sol
    if family == "getrs, one LHS":      # per right-hand side: the factor is read once for all of them
        return 2 * vec, sol
    raise ValueError(family)


def device_time(run, reset, reps=5):
    ts = []
    for _ in range(reps):
        reset()
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); run(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    return float(np.median(ts))


def measure(family, n, count, rng):
    dev = torch.device("cuda")
    sym = family.startswith("sy")
    nlhs = 1 if family == "getrs, one LHS" else count
    A0 = rng.random((n, n, nlhs))
    if sym:
        A0 = 0.5 * (A0 + A0.transpose(1, 0, 2))
    A0 = torch.from_numpy(np.asfortranarray(A0)).to(dev)
    b0 = torch.from_numpy(np.asfortranarray(rng.random((n, count)))).to(dev)
    A = A0.clone(memory_format=torch.preserve_format); b = b0.clone(memory_format=torch.preserve_format)
    ipiv = torch.empty((nlhs, n), dtype=torch.int32, device=dev).t()
    info = torch.empty((nlhs,), dtype=torch.int32, device=dev)

    def reset():
        A.copy_(A0); b.copy_(b0)
    if family == "gesv":
        run = lambda: H.gesv_batched(A, b, ipiv, info)
    elif family == "sysv":
        run = lambda: H.sysv_batched(A, b, ipiv, info)
    elif family == "getrf+getrs":
        run = lambda: (H.getrf_batched(A, ipiv, info), H.getrs_batched(A, ipiv, b))
    elif family == "sytrf+sytrs":
        run = lambda: (H.sytrf_batched(A, ipiv, info), H.sytrs_batched(A, ipiv, b))
    else:
        H.getrf_batched(A0, ipiv, info)
        torch.cuda.synchronize()
        run = lambda: H.getrs_batched(A0, ipiv, b)
    run(); torch.cuda.synchronize()
    return device_time(run, reset)


def numpy_time(n, count, rng):
    A = rng.random((count, n, n)) + n * np.eye(n)
    b = rng.random((count, n, 1))
    t0 = time.perf_counter(); np.linalg.solve(A, b); t1 = time.perf_counter()
    t0b = time.perf_counter(); np.linalg.solve(A, b); t1b = time.perf_counter()
    return min(t1 - t0, t1b - t0b) / count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default=None)
    ap.add_argument("--quick", action="store_true", help="one fixed batch per size, no calibration, no host timings")
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")] if args.sizes else SIZES
    rng = np.random.default_rng(0)
    families = ["gesv", "getrf+getrs", "sysv", "sytrf+sytrs", "getrs, one LHS"]
    lines = []
    cpu_per = {}
    for n in sizes:
        if not args.quick:
            cpu_per[n] = numpy_time(n, int(max(64, min(20000, 2e7 / n ** 3))), rng)
        for fam in families:
            cap = int(max(1, MEM_CAP / (8 * n * n if fam != "getrs, one LHS" else 8 * n)))
            count = int(min(cap, 10 ** 6 if n <= 10 else max(64, 4 * 10 ** 7 // n ** 3)))
            if args.quick:
                count = min(count, 20000)
            t = measure(fam, n, count, rng)
            while not args.quick and t < 100e-6 and count < cap:
                count = int(min(cap, count * max(2.0, 150e-6 / max(t, 1e-7))))
                t = measure(fam, n, count, rng)
            byt, flo = model(fam, n)
            per = t / count
            roof = max(byt / HBM, flo / FP64)
            line = {"family": fam, "n": n, "count": count, "launch_ms": round(t * 1e3, 4), "ns_per_system": round(per * 1e9, 3),
                    "bytes_per_system": byt, "flops_per_system": flo, "roof_fraction": round(roof / per, 4),
                    "bound": "HBM" if byt / HBM >= flo / FP64 else "fp64"}
            if n in cpu_per:
                line["numpy_stacked_solve_ns_per_system"] = round(cpu_per[n] * 1e9, 1)
                line["speedup_vs_numpy"] = round(cpu_per[n] / per, 1)
            lines.append(line)
            print(json.dumps(line), flush=True)
    if not args.quick:
        n, count = 6, 10 ** 6
        A = np.asfortranarray(rng.random((n, n, count))); b = np.asfortranarray(rng.random((n, count)))
        A2, b2 = A.copy(order="F"), b.copy(order="F")
        L.mgeneral(A2, b2)                                     # warm-up (pinned buffers, device buffers)
        ts = []
        for _ in range(3):
            A2, b2 = A.copy(order="F"), b.copy(order="F")
            t0 = time.perf_counter(); L.mgeneral(A2, b2); ts.append(time.perf_counter() - t0)
        byt = model("gesv", n)[0] * count
        line = {"family": "host path mgeneral (PCIe-bound: every byte crosses the host link)", "n": n, "count": count,
                "wall_ms": round(min(ts) * 1e3, 3), "ns_per_system": round(min(ts) / count * 1e9, 3),
                "GB_per_s_over_link": round(byt / min(ts) / 1e9, 2),
                "numpy_stacked_solve_ns_per_system": round(cpu_per.get(6, numpy_time(6, 20000, rng)) * 1e9, 1)}
        lines.append(line)
        print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "lines": lines}, f, indent=1)


if __name__ == "__main__":
    main()
