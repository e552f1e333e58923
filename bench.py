#!/usr/bin/env python3
"""bench.py — whole-job throughput of the WLSQM hot path on N MI355X of one node.

A "step" is one pass of the fused assemble+factor+solve kernel over one batch of synthetic local
fits (inputs resident in HBM before the timed region starts).  Default workload = BASELINE.json
configs[1] ("C2"): 2D order-2, 1M Halton points, 32 nearest neighbours, WEIGHT_CENTER, all DOFs
unknown — that is `value`.  One process per GPU; for N > 1 the driver launches this file under
torch.distributed.run and every rank fits its own 1M-case shard (independent local problems: no
data-path collective, "weak" scaling).

A plain run sets up, warms up, times exactly --steps steps and prints the headline JSON as its only stdout line; its
roofline block comes from HIP events over the timed region itself.  Everything else is measured with `--full` only: the
parity checks against the reference-generated goldens and the CPU oracle, the CPU baseline, dedicated per-kernel timings,
the strict / accurate numerics modes, and every other BASELINE config with the same --steps / --warmup, reported under
"configs" (each with ms_per_step, kernel_ms, roofline fraction, traffic and parity against the reference-generated golden
of that config): C1 at its specified 10k points and at a working set beyond the Infinity Cache, C3, C4 (ExpertSolver,
256 stacked right-hand sides), C5 at 1M and at the full 16M points of configs[4] on one GPU, and the literal form of
configs[4] (`--config C5 --sharded`: ONE Morton-ordered cloud partitioned over the ranks, own-points-only neighbour
search against a halo band, index-based fit, halo values exchanged per step on a side stream under the interior fits;
wlsqm/sharded.py HaloCloudSolver).  `--config Cx` measures one config as `value` instead.

`--dump-outputs DIR` writes what the timed path returned in its last timed step as DIR/<name>.npy (float64, at most
64 MB in all: a fixed, seeded sample of the rows of a larger output).  The inputs are synthetic and seeded, so two builds
run with the same arguments can be compared output for output.

With `--full`, rank 0 prints the full record on a line prefixed "# full: " and then, as the LAST line of stdout, the compact
headline JSON (< 1.5 KB: the contract's fields + roofline + cpu_baseline + a parity digest + one [ms, frac] pair per side config).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "python-wlsqm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import synth  # noqa: E402

# BASELINE.json configs -> (dim, order, nk, weighting, knowns); B_fit from SURVEY.md §8d
CONFIGS = {
    "C1": dict(dim=1, order=2, nk=8, wm=1, knowns=0, desc="1D order-2, 8 neighbours, WEIGHT_UNIFORM"),
    "C2": dict(dim=2, order=2, nk=32, wm=2, knowns=0, desc="2D order-2, Halton, 32 neighbours, WEIGHT_CENTER, all DOFs unknown"),
    "C3": dict(dim=2, order=4, nk=64, wm=2, knowns=1, desc="2D order-4, Halton, 64 neighbours, WEIGHT_CENTER, F known"),
    "C5": dict(dim=3, order=2, nk=40, wm=2, knowns=0, desc="3D order-2, Halton, 40 neighbours, WEIGHT_CENTER, all DOFs unknown"),
    # BASELINE configs[3]: the C2 geometry prepared once in an ExpertSolver, then many right-hand sides (measure_c4 below)
    "C4": dict(dim=2, order=2, nk=32, wm=2, knowns=0, desc="ExpertSolver, 2D order-2, Halton, 32 neighbours: prepare once + stacked right-hand sides"),
}
NDOF = {1: [1, 2, 3, 4, 5], 2: [1, 3, 6, 10, 15], 3: [1, 4, 10, 20, 35]}
HBM_PEAK_GBPS = 8000.0     # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
FP64_PEAK_TFLOPS = 78.6    # vector fp64 peak; measured: a lone wave per SIMD issues 62, four waves 74 (tools/ubench/fp64_issue.hip)
GOLDEN_OF = {"C2": "C2_1M", "C3": "C3_1M", "C5": "C5_1M"}      # reference outputs at the density the metric is quoted on
DUMP_LIMIT = 64 * 2 ** 20  # bytes: --dump-outputs writes at most this much in all


def dump_sample(t, axis=0, limit=DUMP_LIMIT):
    """The device tensor t as a float64 host array; when it is larger than `limit`, a fixed, seeded sample of its entries
    along `axis` (sorted indices, the same for every run with the same shape)."""
    import torch
    n = t.shape[axis]
    row = t.numel() // max(1, n) * 8
    if n * row > limit:
        idx = np.sort(np.random.default_rng(0).choice(n, max(1, limit // row), replace=False))
        t = t.index_select(axis, torch.from_numpy(idx).to(t.device))
    return t.to(torch.float64).cpu().numpy()


def dump_outputs(d, outputs):
    """--dump-outputs: one DIR/<name>.npy per array the timed path returned in its last step."""
    os.makedirs(d, exist_ok=True)
    for name, arr in outputs.items():
        np.save(os.path.join(d, name + ".npy"), np.ascontiguousarray(arr, dtype=np.float64))


def bytes_per_fit(dim, order, nk, knowns):
    """Algorithmic HBM bytes per fit, dense reference layout:
    8 nk (dim+1) [xk+fk] + 8 dim [xi] + 8 no [fi out] + 8 popcount(knowns) [fi in] + 20 [nk, order, knowns, wm]."""
    no = NDOF[dim][order]
    return 8 * nk * (dim + 1) + 8 * dim + 8 * no + 8 * bin(knowns).count("1") + 20


def bytes_per_fit_indexed(dim, order, nk):
    """Index-based input (reported separately): 4 nk [hoods] + 8 (dim+1) [the point's own row of S and F]
    + 8 no [fi] + 20."""
    return 4 * nk + 8 * (dim + 1) + 8 * NDOF[dim][order] + 20


def flops_per_fit(dim, order, nk, knowns):
    """fp64 operations per fit of the moment-form kernels (FMA = 2): per neighbour the offsets and squared distance
    (3 dim - 1), the weight (23: a reciprocal-square-root seeded root, two Newton steps, the quadratic), the monomial
    powers and the distinct moments of the matrix and of the right-hand side (one FMA each); per case the expansion of
    the no(no+1)/2 entries, the LDL^T factorisation (no^3 / 3) and the two substitutions (2 no^2)."""
    no = NDOF[dim][order]
    D = 2 * order
    nmom = {1: D + 1, 2: (D + 1) * (D + 2) // 2, 3: (D + 1) * (D + 2) * (D + 3) // 6}[dim]
    per_nb = (3 * dim - 1) + 23 + dim * D + 2 * (nmom + no)
    return nk * per_nb + no * (no + 1) // 2 + no ** 3 // 3 + 2 * no * no


def sweep_flops(dim, order, nk):
    """fp64 operations of ONE refinement sweep of solve_iterative (impl.pyx:986-1083; FMA = 2): per neighbour the offsets (dim), the Taylor
    model by Horner's rule (2 no), the residual (1), its weighted right-hand-side moments (1 + 2 no) and the norm (1); per case the two
    substitutions with the stored factor (2 no^2) and the update (no)."""
    no = NDOF[dim][order]
    return nk * (dim + 4 * no + 3) + 2 * no * no + no


def load_traffic(config, units_per_launch):
    """HBM bytes per launch from the committed PMC summary (profiles/traffic_<config>.json, tools/make_traffic.py) and the
    file it came from, or (None, None) when there is none for this config / launch size.  This is a RECORDED measurement
    of the same kernel at the same launch size (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes), not something this run
    measures: PMC collection needs the profiler."""
    name = "traffic_%s.json" % config
    try:
        t = json.load(open(os.path.join(ROOT, "profiles", name)))
        if int(units_per_launch) in (int(t.get("cases_per_launch", -1)), int(t.get("units_per_launch", -1))):      # (C4: units = cases x stacked right-hand sides)
            return t.get("hbm_bytes_per_launch"), "profiles/" + name
    except Exception:
        pass
    return None, None


def load_valu_busy(config):
    """VALU-busy fraction of the dominant kernel from the committed SQ counter pass (profiles/*_<config>_pmc_summary.json)."""
    import glob
    best = None
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_%s_pmc_summary.json" % config))):
        try:
            ks = json.load(open(f))["kernels"]
            v = max((k["derived"].get("valu_busy", 0.0) for k in ks.values()), default=None)
            if v:
                best = (v, "profiles/" + os.path.basename(f))
        except Exception:
            pass
    return best or (None, None)


def build_problem(cfg, ncases, rank, device=None):
    """Synthetic inputs of SURVEY.md section 8d: Halton points, nk nearest neighbours (self excluded), smooth field.
    With `device` (a torch device) the neighbour search runs on that GPU (wlsqm.hip.knn, exact, same neighbours as
    cKDTree up to the order inside last-ulp distance ties); otherwise scipy's cKDTree on the host."""
    dim, nk = cfg["dim"], cfg["nk"]
    if dim == 1:
        p = synth.line_problem_1d(ncases, nk // 2, seed=rank)
        return p["S"], p["F"], p["hoods"]
    S = synth.halton(ncases, dim, skip=1 + rank * ncases)       # each rank owns a different stretch of the sequence
    F = synth.field(S)
    if device is not None:
        import torch
        import wlsqm.hip as whip
        hoods = whip.knn(torch.from_numpy(S).to(device), nk).cpu().numpy()
        return S, F, hoods
    world = int(os.environ.get("WORLD_SIZE", "1"))
    hoods = synth.knn(S, nk, workers=max(1, len(os.sched_getaffinity(0)) // world))
    return S, F, hoods


class Timer:
    """The timed region of the contract: W untimed steps, then exactly K steps bracketed by barrier + synchronize, MAX over ranks."""

    def __init__(self, dist, dev):
        self.dist, self.dev = dist, dev

    def barrier(self):
        import torch
        torch.cuda.synchronize()
        if self.dist is not None:
            self.dist.barrier()
            torch.cuda.synchronize()

    def run(self, step, steps, warmup, wake_s=0.3, collective=False):
        import torch
        # The GPU sat idle through the setup and has dropped to its low power state; the first ~50 ms of kernels run at
        # reduced clocks (measured: 0.214 ms vs 0.183 ms per step).  Bring it back to the clocks of a long-running job before
        # the untimed warm-up, so a short --warmup does not measure the ramp.  Steps that contain a collective run a fixed
        # count instead (the same on every rank).
        if collective and self.dist is not None:
            for _ in range(200):
                step()
            torch.cuda.synchronize()
        else:
            t_wake = time.perf_counter()
            while time.perf_counter() - t_wake < wake_s:
                for _ in range(8):
                    step()
                torch.cuda.synchronize()
        for _ in range(warmup):
            step()
        self.barrier()
        # HIP events over the SAME timed region, on the stream the kernels are launched on (the library launches on torch's current
        # stream): event span / steps = the average launch duration inside the region (this rank's own)
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(steps):
            step()
        e1.record()
        self.barrier()
        dt = time.perf_counter() - t0
        self.last_event_ms_per_step = e0.elapsed_time(e1) / max(1, steps)
        if self.dist is not None:
            t = torch.tensor([dt], dtype=torch.float64, device=(self.dev if self.dist.get_backend() == "nccl" else "cpu"))
            self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt


def golden_parity_c1(dev):
    """C1 (BASELINE configs[0]) against the reference: the first 512 cases of the specified 10 000-point cloud, outputs captured
    from the reference's fit_1D_many (tests/golden/config_C1.npz)."""
    import torch
    import _cases
    import _parity
    import wlsqm.hip as whip
    from oracle import oracle
    c = _cases.config("C1")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    fi_d = t(c["fi0"])
    whip.fit_many_device(1, c["order"], t(c["xk"]), t(c["fk"]), t(c["nk_a"]), t(c["xi"]), fi_d, t(c["knowns_a"]), t(c["wm_a"]))
    torch.cuda.synchronize()
    kernel = whip.last_kernel()
    fi_o = c["fi0"].copy()
    oracle.fit_many(1, c["xk"], c["fk"], c["nk_a"], c["xi"], fi_o, None, 0, c["order_a"], c["knowns_a"], c["wm_a"], ntasks=8)
    truth = _parity.truth_fit(1, c["xk"], c["fk"], c["nk_a"], c["xi"], c["fi0"], c["order_a"], c["knowns_a"], c["wm_a"])
    acc = _parity.accounting(fi_d.cpu().numpy(), c["g"]["fi"], truth=truth, oracle=fi_o, conds=c["g"]["conds"])
    acc["golden"] = "tests/golden/config_C1.npz"
    acc["kernel"] = kernel
    return acc


def golden_parity(name, dev):
    """Parity of the device-resident fast kernel against the REFERENCE at the density the metric is quoted on: the 1 024
    cases of tests/golden/config_<name>.npz (every 977th case of the full cloud; inputs rebuilt bit-for-bit, outputs
    captured from the reference's fit_*_many_parallel and ExpertSolver(debug=True).conds() by tests/golden/make_golden.py).
    Strict-1e-10 accounting as in tests/_parity.accounting."""
    import torch
    import _cases
    import _parity
    import wlsqm.hip as whip
    from oracle import oracle
    c = _cases.config_dense(name)
    dim, order, no = c["dim"], c["order"], c["no"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    xk = c["xk"] if dim > 1 else c["xk"][..., 0]
    fi_d = t(c["fi0"])
    whip.fit_many_device(dim, order, t(xk), t(c["fk"]), t(c["nk_a"]), t(c["xi"]), fi_d, t(c["knowns_a"]), t(c["wm_a"]))
    torch.cuda.synchronize()
    kernel = whip.last_kernel()
    fi = fi_d.cpu().numpy()
    kn = int(c["knowns_a"][0])
    known_cols = [a for a in range(no) if (kn >> a) & 1]
    fi_o = c["fi0"].copy()
    oracle.fit_many(dim, c["xk"], c["fk"], c["nk_a"], c["xi"], fi_o, None, 0, c["order_a"], c["knowns_a"], c["wm_a"], ntasks=8)
    truth = _parity.truth_fit(dim, c["xk"], c["fk"], c["nk_a"], c["xi"], c["fi0"], c["order_a"], c["knowns_a"], c["wm_a"])
    acc = _parity.accounting(fi, c["g"]["fi"], truth=truth, oracle=fi_o, conds=c["conds"], known_cols=known_cols)
    acc["golden"] = "tests/golden/config_%s.npz" % name
    acc["kernel"] = kernel
    acc["knowns_bit_identical"] = bool(all(np.array_equal(fi[:, a], c["fi0"][:, a]) for a in known_cols))
    # the same cases in the reference-order numerics mode (csrc/fit_strict.hip): bit-identical to the oracle by construction,
    # so its distance to the reference is LAPACK's summation order and nothing else
    fi_s = t(c["fi0"])
    whip.fit_many_device(dim, order, t(xk), t(c["fk"]), t(c["nk_a"]), t(c["xi"]), fi_s, t(c["knowns_a"]), t(c["wm_a"]), strict=True)
    torch.cuda.synchronize()
    fi_s = fi_s.cpu().numpy()
    cols = [m for m in range(no) if m not in known_cols]
    Es = _parity.column_metric(fi_s, c["g"]["fi"])
    acc["strict_mode"] = {"kernel": whip.last_kernel(), "E": [float(Es[m]) for m in cols], "E_max": float(max(Es[m] for m in cols)),
                          "strict_1e-10_columns": int(sum(Es[m] <= 1e-10 for m in cols)), "columns": len(cols),
                          "bit_identical_to_oracle": bool(np.array_equal(fi_s, fi_o))}
    # ... and in the ACCURATE mode (csrc/fit_accurate.hip: the reference's arithmetic with the normal matrix assembled from its upper
    # triangle; round 4, VERDICT r3 item 2: one mode that is within 1e-10 of the reference on every column AND at the roofline's scale)
    if dim > 1 and no <= 10:
        fi_a = t(c["fi0"])
        whip.fit_many_device(dim, order, t(xk), t(c["fk"]), t(c["nk_a"]), t(c["xi"]), fi_a, t(c["knowns_a"]), t(c["wm_a"]), strict="accurate")
        torch.cuda.synchronize()
        ka = whip.last_kernel()
        fi_a = fi_a.cpu().numpy()
        Ea = _parity.column_metric(fi_a, c["g"]["fi"])
        fi_v = np.ascontiguousarray(c["fi0"].copy())                 # its CPU statement: oracle/variants.c with V_SYM
        oracle.variant_fit_many(dim, order, np.ascontiguousarray(c["xk"]), np.ascontiguousarray(c["fk"]), c["nk_a"],
                                np.ascontiguousarray(c["xi"]), fi_v, c["knowns_a"], c["wm_a"], flags=oracle.V_SYM)
        want = fi_v if kn == 0 else fi_o                              # (cases with a known DOF run the strict kernels)
        acc["accurate_mode"] = {"kernel": ka, "E": [float(Ea[m]) for m in cols], "E_max": float(max(Ea[m] for m in cols)),
                                "strict_1e-10_columns": int(sum(Ea[m] <= 1e-10 for m in cols)), "columns": len(cols),
                                "margin_to_1e-10": float(1e-10 / max(Ea[m] for m in cols)),
                                "bit_identical_to_cpu_statement": bool(np.array_equal(fi_a, want))}
    return acc


def measure_fit(name, cfg, n, dev, timer, steps, warmup, rank, parity=True, keep=False, extras=None, unsorted=False, full=True, dump=False):
    """One BASELINE config through the device-resident dense API: build, time, roofline, parity.
    extras: None (basic fit), "sens" (do_sens: + 8 nk no bytes written per fit) or "iter" (iterative refinement, max_iter 10).
    unsorted: every case's neighbours in random order (what a ball query or any caller that does not sort by distance hands over).
    full: also time the launch in a dedicated run (otherwise kernel_ms is the event span of the timed region).
    dump: res["_outputs"] holds what the last timed step returned (fi)."""
    import torch
    import wlsqm.hip as whip
    dim, order, nk = cfg["dim"], cfg["order"], cfg["nk"]
    no = NDOF[dim][order]
    S, F, hoods = build_problem(cfg, n, rank, device=dev)
    # device-resident inputs in the reference's dense layout: xk = S[hoods], fk = F[hoods]  (gathered on the GPU)
    S_d = torch.from_numpy(np.ascontiguousarray(S)).to(dev)
    F_d = torch.from_numpy(F).to(dev)
    h_d = torch.from_numpy(hoods).to(dev)
    if unsorted:
        g = torch.Generator(device=dev); g.manual_seed(11 + rank)
        h_d = torch.gather(h_d, 1, torch.argsort(torch.rand(h_d.shape, device=dev, generator=g), dim=1)).contiguous()
    chunk = 2_000_000
    xk_d = torch.empty((n, nk) + ((dim,) if dim > 1 else ()), dtype=torch.float64, device=dev)
    fk_d = torch.empty((n, nk), dtype=torch.float64, device=dev)
    for j0 in range(0, n, chunk):                      # chunked: the int64 index tensor of 16M x 40 would be 5 GB
        hh = h_d[j0:j0 + chunk].long()
        xk_d[j0:j0 + chunk] = S_d[hh]; fk_d[j0:j0 + chunk] = F_d[hh]
        del hh
    xi_d = S_d.clone()
    fi_d = torch.zeros((n, no), dtype=torch.float64, device=dev)
    fi_d[:, 0] = F_d
    nk_d = torch.full((n,), nk, dtype=torch.int32, device=dev)
    kn_d = torch.full((n,), cfg["knowns"], dtype=torch.int64, device=dev)
    wm_d = torch.full((n,), cfg["wm"], dtype=torch.int32, device=dev)
    del h_d
    args = (dim, order, xk_d, fk_d, nk_d, xi_d, fi_d, kn_d, wm_d)
    if extras:
        # the fit with sensitivities / refinement / in the accurate numerics mode is one or several kernels per call: the whole call is timed
        # with events on its stream
        kw = (dict(sens=torch.zeros((n, nk, no), dtype=torch.float64, device=dev)) if extras == "sens" else
              dict(strict="accurate") if extras == "accurate" else dict(iterative=True, max_iter=10))
        dt = timer.run(lambda: whip.fit_many_device(*args, **kw), steps, warmup)
        kernel = whip.last_kernel()
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        reps = min(max(steps, 5), 50)
        e0.record()
        for _ in range(reps):
            whip.fit_many_device(*args, **kw)
        e1.record(); torch.cuda.synchronize()
        ms_kernel = e0.elapsed_time(e1) / reps
        B_fit = bytes_per_fit(dim, order, nk, cfg["knowns"]) + (8 * nk * no if extras == "sens" else 0)
        achieved = B_fit * n / (ms_kernel * 1e-3) / 1e9
        res = {"workload": "%s with %s: %s%s; %d local fits per GPU per step, device-resident dense xk/fk"
                           % (name, {"sens": "sensitivities (do_sens)", "accurate": "the ACCURATE numerics mode (reference arithmetic, mirrored triangle)"}.get(
                               extras, "iterative refinement (max_iter 10)"), cfg["desc"], ", neighbours in RANDOM order" if unsorted else "", n),
               "fits_per_gpu": n, "bytes_per_fit": B_fit, "ms_per_step": dt / steps * 1e3, "fits_per_s": n * steps / dt,
               "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBPS,
                            "traffic": None, "kernel_ms": ms_kernel, "kernel": kernel, "algorithmic_bytes_per_launch": B_fit * n,
                            "note": "whole call (every kernel of the path), HIP events on the launch stream"}}
        if extras == "iter":
            # where the roof is: sweeps per case from the CPU port on a sample (the stop rule is an exact equality of two
            # residual norms, impl.pyx:1057: counts differ by a sweep between implementations, their distribution does not), the arithmetic of
            # the call against the fp64 vector peak, and the bytes of the rows the sweeps read again (from L2 / the Infinity Cache, not HBM)
            sw = None
            if parity and rank == 0:
                from oracle import oracle
                m = 256
                xk, fk, xi = (a[:m].cpu().numpy() for a in (xk_d, fk_d, xi_d))
                its = []
                for j in range(m):
                    fij = np.zeros((1, no)); fij[0, 0] = F[j]
                    its.append(oracle.fit_many(dim, xk[j:j + 1], fk[j:j + 1], np.full(1, nk, np.int32), xi[j:j + 1], fij, None, 0, np.full(1, order, np.int32),
                                               np.full(1, cfg["knowns"], np.int64), np.full(1, cfg["wm"], np.int32), iterative=True, max_iter=10))
                sw = {"cases": m, "mean": float(np.mean(its)), "max": int(np.max(its)), "min": int(np.min(its)), "source": "CPU port, one case per call"}
            mean_sw = sw["mean"] if sw else 10.0
            fl = flops_per_fit(dim, order, nk, cfg["knowns"]) + mean_sw * sweep_flops(dim, order, nk)
            tf = fl * n / (ms_kernel * 1e-3) / 1e12
            res["roofline"].update({"valu_flop_per_fit": fl, "valu_achieved_tflops": tf, "valu_peak_tflops": FP64_PEAK_TFLOPS, "valu_frac": tf / FP64_PEAK_TFLOPS,
                                    "sweeps_per_case": sw, "rows_reread_bytes_per_fit": mean_sw * 8.0 * nk * (dim + 1),
                                    "note": res["roofline"]["note"] + "; valu_frac counts the fit and the MEAN number of sweeps (a wave runs the maximum over its 64 cases)"})
        if extras == "accurate" and parity and rank == 0:
            # the first 1 024 cases against the mode's CPU statement (variants.c V_SYM: bit for bit) and against the CPU port of the reference
            from oracle import oracle
            m = 1024
            xk, fk, xi = (a[:m].cpu().numpy() for a in (xk_d, fk_d, xi_d))
            got = fi_d[:m].cpu().numpy()
            kn = np.full(m, cfg["knowns"], np.int64); wm = np.full(m, cfg["wm"], np.int32); nka = np.full(m, nk, np.int32)
            sym = np.zeros((m, no)); sym[:, 0] = F[:m]
            oracle.variant_fit_many(dim, order, xk, fk, nka, xi, sym, kn, wm, flags=oracle.V_SYM)
            ref = np.zeros((m, no)); ref[:, 0] = F[:m]
            oracle.fit_many(dim, xk, fk, nka, xi, ref, None, 0, np.full(m, order, np.int32), kn, wm, ntasks=8)
            scale = np.abs(ref).max(axis=0)
            E = np.abs(got - ref).max(axis=0) / np.where(scale > 0, scale, 1.0)
            res["parity"] = {"vs_cpu_statement": {"cases": m, "bit_identical_cases": int((got.view(np.int64) == sym.view(np.int64)).all(axis=1).sum())},
                             "vs_oracle": {"cases": m, "E_max": float(E.max()), "columns": int(no), "columns_le_1e-10": int((E <= 1e-10).sum())}}
        return res, dt
    hint = whip.row_hint(sorted=not unsorted)                         # (the caller's word about its rows: wlsqm_hip_set_order_hint)
    hint.__enter__()
    dt = timer.run(lambda: whip.fit_many_device(*args), steps, warmup)
    kernel = whip.last_kernel()
    outputs = {"fi": dump_sample(fi_d)} if dump else None
    # dominant kernel: HIP events over the timed region itself (Timer.run), on the stream it is launched on; with `full`, a dedicated run of
    # the same launch (events inside the library, no Python between the launches) is kept beside it in the full record
    ms_region = getattr(timer, "last_event_ms_per_step", None)
    ms_dedicated = whip.time_fit_device(*args, reps=min(max(steps, 20), 500)) if full else None
    hint.__exit__()
    launch_bound = full and ((not ms_region) or ms_region > 1.5 * ms_dedicated)          # tiny launches: the span measures Python's launch rate, not the kernel
    ms_kernel = ms_dedicated if launch_bound else ms_region
    B_fit = bytes_per_fit(dim, order, nk, cfg["knowns"])
    achieved = B_fit * n / (ms_kernel * 1e-3) / 1e9
    working_set = B_fit * n
    traffic, tsrc = load_traffic(name, n)
    roof = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBPS,
            "traffic": traffic, "traffic_source": tsrc, "kernel_ms": ms_kernel, "kernel": kernel,
            "algorithmic_bytes_per_launch": working_set, "kernel_ms_source": ("dedicated run (the timed region is launch-bound)" if launch_bound else "HIP events over the timed region / steps"),
            "kernel_ms_dedicated_run": ms_dedicated}
    if working_set < 256 * 2 ** 20:
        roof["note"] = ("working set %.0f MB fits the 256 MB Infinity Cache: back-to-back launches re-read it on-die, so this is a "
                        "cache-resident rate, not an HBM fraction" % (working_set / 1e6))
    if name == "C2":
        # a bare streaming kernel with this kernel's read : write mix (16 : 1) and launch size, measured once (tools/ubench/hbm_mix.hip)
        roof.update({"bare_stream_same_mix_GBps": [5560.0, 5720.0], "bare_stream_source": "profiles/r03j_ubench_hbm_mix.txt",
                     "frac_of_bare_stream": achieved / 5720.0})
    if name == "C3" or NDOF[dim][order] >= 15:
        fl = flops_per_fit(dim, order, nk, cfg["knowns"])
        tf = fl * n / (ms_kernel * 1e-3) / 1e12
        vb, vsrc = load_valu_busy("C3") if name == "C3" else (None, None)
        roof.update({"valu_flop_per_fit": fl, "valu_achieved_tflops": tf, "valu_peak_tflops": FP64_PEAK_TFLOPS,
                     "valu_frac": tf / FP64_PEAK_TFLOPS, "valu_busy_pmc": vb, "valu_busy_source": vsrc})
    res = {"workload": "%s: %s%s; %d local fits per GPU per step, device-resident dense xk/fk" % (name, cfg["desc"], ", neighbours in RANDOM order" if unsorted else "", n),
           "fits_per_gpu": n, "bytes_per_fit": B_fit, "ms_per_step": dt / steps * 1e3, "fits_per_s": n * steps / dt,
           "roofline": roof}
    if parity and rank == 0 and name in GOLDEN_OF:
        res["parity"] = {"vs_reference_golden": golden_parity(GOLDEN_OF[name], dev)}
        # what the reference-order mode costs on the full batch (a validation mode: never the `value`)
        with whip.strict():
            ms_strict = whip.time_fit_device(*args, reps=3)
        sm = res["parity"]["vs_reference_golden"]["strict_mode"]
        sm["ms_per_step"] = ms_strict
        sm["slowdown_vs_fast"] = ms_strict / ms_kernel
        res["parity"]["strict_mode"] = sm
        am = res["parity"]["vs_reference_golden"].get("accurate_mode")
        if am:
            with whip.accurate():
                # (three measurements of as many launches as the headline's timed region; the mode's kernel runs at the edge of the clocks the box
                # sustains: one box gave 0.245-0.268 ms within one minute, tools/time_accurate_reps.py — the median is reported, the best beside it)
                acc_ms = sorted(whip.time_fit_device(*args, reps=20) for _ in range(3))
            ms_acc = acc_ms[1]
            am["ms_per_step"] = ms_acc                                # the WHOLE call: the speculative kernel + its (idle) clean-up kernel
            am["ms_best_of_3"] = acc_ms[0]
            am["slowdown_vs_fast"] = ms_acc / ms_kernel
            am["frac"] = B_fit * n / (ms_acc * 1e-3) / (HBM_PEAK_GBPS * 1e9)
            res["parity"]["accurate_mode"] = am
    elif parity and rank == 0 and name == "C1":
        res["parity"] = {"vs_reference_golden": golden_parity_c1(dev)}
    if keep:
        res["_tensors"] = dict(xk=xk_d, fk=fk_d, xi=xi_d, fi=fi_d, F=F)
    if outputs:
        res["_outputs"] = outputs
    return res, dt


def measure_c4(cfg, n, R, dev, timer, steps, warmup, rank, parity=True, full=True, dump=False):
    """BASELINE configs[3]: ExpertSolver on the C2 geometry, prepare once, then right-hand sides F_t = sin(pi x + 0.01 t)
    cos(pi y).  A step = ONE solve_many_device call over R stacked fields; a fit = one (case, field)
    pair.  Algorithmic bytes per fit: fk 8 nk + fi 8 no + the case's [nr x nk] solution operator shared by
    the R fields of a step (310 B at R = 256; the stored operator has 16 rows per case, so the measured traffic is a little
    higher).  The time-stepping rate (one fused solve_device launch per field, 852 B per fit) is reported beside it."""
    import torch
    import wlsqm
    import wlsqm.hip as whip
    dim, order, nk = cfg["dim"], cfg["order"], cfg["nk"]
    no = NDOF[dim][order]
    S, F, hoods = build_problem(cfg, n, rank, device=dev)
    solver = wlsqm.ExpertSolver(dimension=dim, nk=np.full(n, nk, np.int32), order=np.full(n, order, np.int32),
                                knowns=np.full(n, cfg["knowns"], np.int64),
                                weighting_method=np.full(n, cfg["wm"], np.int32))
    S_d = torch.from_numpy(S).to(dev)
    h_d = torch.from_numpy(hoods.astype(np.int64)).to(dev)
    t0 = time.perf_counter()
    solver.prepare_device(S_d, S_d[h_d].contiguous())
    torch.cuda.synchronize()
    t_prepare = time.perf_counter() - t0
    fk = torch.empty((R, n, nk), dtype=torch.float64, device=dev)
    for r in range(R):
        fk[r] = (torch.sin(np.pi * S_d[:, 0] + 0.01 * r) * torch.cos(np.pi * S_d[:, 1]))[h_d]
    fi = torch.zeros((R, n, no), dtype=torch.float64, device=dev)
    # the stored solution operator of the geometry: built ONCE per prepare() (sensitivities of every case + transpose), timed here
    # on its own; `value` is the rate of the solves with the operator in place, `value_including_prepare` charges the build to ONE
    # step of R fields (the worst case: a geometry that is used for a single stack)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    built = solver.prepare_operator()
    torch.cuda.synchronize()
    t_operator = time.perf_counter() - t0
    dt = timer.run(lambda: solver.solve_many_device(fk, fi), steps, warmup)
    kernel = whip.last_kernel()
    outputs = {"fi": dump_sample(fi, axis=1)} if dump else None
    ms_kernel = getattr(timer, "last_event_ms_per_step", None)
    ms_step_field = None
    if full:
        # the kernel alone, events on the stream it is launched on (torch's current stream is passed to the launch)
        reps = min(max(steps, 5), 50)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            solver.solve_many_device(fk, fi)
        e1.record(); torch.cuda.synchronize()
        ms_kernel = e0.elapsed_time(e1) / reps
        # time stepping: one fused launch per field
        fi_seq = torch.zeros_like(fi[0])
        e0.record()
        for r in range(min(R, 64)):
            solver.solve_device(fk[r], fi_seq)
        e1.record(); torch.cuda.synchronize()
        ms_step_field = e0.elapsed_time(e1) / min(R, 64)
    nr = no - bin(cfg["knowns"]).count("1")
    B_fit = 8 * nk + 8 * no + 8 * nr * nk / R       # fk + fi + the case's [nr x nk] operator shared by the R fields
    achieved = B_fit * n * R / (ms_kernel * 1e-3) / 1e9
    traffic, tsrc = load_traffic("C4", n * R)
    res = {"workload": "C4: %s; %d cases x %d stacked fields per GPU per step (a fit = one case of one field), "
                       "geometry and fields device-resident" % (cfg["desc"], n, R),
           "fits_per_gpu": n * R, "nrhs": R, "bytes_per_fit": B_fit, "prepare_ms_device_arrays": t_prepare * 1e3,
           "prepare_operator_ms": t_operator * 1e3, "operator_built": bool(built),
           "ms_per_step": dt / steps * 1e3, "fits_per_s": n * R * steps / dt,
           "value_including_prepare": n * R / (dt / steps + t_operator + t_prepare),
           "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                        "frac": achieved / HBM_PEAK_GBPS, "traffic": traffic, "traffic_source": tsrc, "kernel_ms": ms_kernel,
                        "kernel": kernel, "algorithmic_bytes_per_launch": B_fit * n * R}}
    if full:
        res["time_stepping"] = {"ms_per_field": ms_step_field, "fits_per_s": n / (ms_step_field * 1e-3),
                                "bytes_per_fit": bytes_per_fit(dim, order, nk, cfg["knowns"])}
    else:
        res["roofline"]["note"] = "kernel_ms: HIP events over the timed region / steps"
    if parity and rank == 0:
        # the last field of the stack against the oracle and the 80-bit solution (the reference has no stacked solve: its
        # ExpertSolver.solve is called once per field, expert.pyx:537-571; the golden of this geometry is C2's)
        from oracle import oracle
        import _parity
        ns = min(n, 1024)
        r = R - 1
        xk_h = S[hoods[:ns]]; fk_h = fk[r, :ns].cpu().numpy(); xi_h = S[:ns]
        fi_o = np.zeros((ns, no)); fi_in = fi_o.copy()
        meta = (np.full(ns, nk, np.int32), np.full(ns, order, np.int32), np.full(ns, cfg["knowns"], np.int64),
                np.full(ns, cfg["wm"], np.int32))
        oracle.fit_many(dim, xk_h, fk_h, meta[0], xi_h, fi_o, None, 0, meta[1], meta[2], meta[3], ntasks=8)
        truth = _parity.truth_fit(dim, xk_h, fk_h, meta[0], xi_h, fi_in, meta[1], meta[2], meta[3])
        fi_seq2 = torch.zeros_like(fi[0])
        solver.solve_device(fk[r], fi_seq2)
        torch.cuda.synchronize()
        acc = _parity.accounting(fi[r, :ns].cpu().numpy(), fi_o, truth=truth)
        acc["reference"] = "CPU oracle on the first %d cases of field %d (the reference has no stacked solve)" % (ns, r)
        acc["max_rel_diff_to_sequential_solve_device"] = float(((fi[r] - fi_seq2).abs().amax(0) / fi_seq2.abs().amax(0)).max())
        res["parity"] = {"vs_oracle": acc}
    del fk, fi
    if outputs:
        res["_outputs"] = outputs
    return res, dt


def halton_device(n, dim, dev, skip=1):
    """synth.halton on the GPU (same operations in the same order per point: bit-identical), for the 16M-point cloud."""
    import torch
    idx = torch.arange(skip, skip + n, dtype=torch.int64, device=dev)
    out = torch.empty((n, dim), dtype=torch.float64, device=dev)
    for d in range(dim):
        b = (2, 3, 5)[d]
        i = idx.clone(); f = 1.0
        r = torch.zeros(n, dtype=torch.float64, device=dev)
        while bool((i > 0).any()):
            f = f / b
            r += f * (i % b).to(torch.float64)
            i //= b
        out[:, d] = r
    return out


def morton_order_device(S, bits=16):
    """synth.morton_order on the GPU."""
    import torch
    q = (S * (1 << bits)).to(torch.int64).clamp_(0, (1 << bits) - 1)
    dim = S.shape[1]
    key = torch.zeros(S.shape[0], dtype=torch.int64, device=S.device)
    for b in range(bits):
        for d in range(dim):
            key |= ((q[:, d] >> b) & 1) << (b * dim + d)
    return torch.argsort(key, stable=True)


def run_sharded(a, dev, dist, rank, world, timer, parity=True, dump=False):
    """BASELINE configs[4] in its literal form: ONE 3D cloud of world x --ncases Morton-ordered Halton points, partitioned over
    the ranks in contiguous blocks; every rank searches only its own points (against a verified halo band), fits them with the
    index-based kernel from its local tables and, per step, receives only the halo values it names (all_to_all_single on a side
    stream, overlapped with the interior fits).  A step = exchange + fit of every point + an explicit update of the field
    (F <- fitted value + 1e-7 x fitted Laplacian).  value = points of the whole cloud x steps / time."""
    import torch
    import wlsqm.hip as whip
    from wlsqm.sharded import HaloCloudSolver, case_range
    cfg = CONFIGS["C5"]
    dim, order, nk = cfg["dim"], cfg["order"], cfg["nk"]
    no = NDOF[dim][order]
    n_local = a.ncases
    N = n_local * world
    t0 = time.perf_counter()
    # the synthetic cloud: every rank generates the Halton points, orders them along the Morton curve and KEEPS ITS BLOCK ONLY;
    # the solver is handed that block and finds its halo band by exchanging boxes and band points with the other ranks
    S = halton_device(N, dim, dev)
    lo, hi = case_range(N, rank, world)
    own = S[morton_order_device(S)[lo:hi]].contiguous()
    del S
    torch.cuda.empty_cache()
    solver = HaloCloudSolver(dim, own, nk, order=order, knowns=cfg["knowns"], weighting_method=cfg["wm"], device=dev,
                             own_range=(lo, N))
    solver.set_own_values(torch.sin(np.pi * own[:, 0]) * torch.cos(np.pi * own[:, 1]) * torch.exp(own[:, 2]))
    del own
    torch.cuda.synchronize()
    t_setup = time.perf_counter() - t0

    last = [None]

    def step():
        fi = last[0] = solver.step()
        solver.values[: solver.n_own] = fi[:, 0] + 1e-7 * (fi[:, 4] + fi[:, 6] + fi[:, 8])      # i3_X2, i3_Y2, i3_Z2
    dt = timer.run(step, a.steps, a.warmup, collective=True)
    kernel = whip.last_kernel()
    outputs = ({"fi": dump_sample(last[0], limit=DUMP_LIMIT * 3 // 4), "values": dump_sample(solver.values[: solver.n_own], limit=DUMP_LIMIT // 4)}
               if dump else None)
    # the two parts alone (events on the launch stream): fits without the exchange, exchange without the fits
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    reps = max(3, min(a.steps, 20))
    timer.barrier()
    ev[0].record()
    for _ in range(reps):
        solver.fit_interior(); solver.fit_boundary()
    ev[1].record(); torch.cuda.synchronize()
    timer.barrier()
    ev[2].record()
    for _ in range(reps):
        solver.exchange_begin(); solver.exchange_end()
    ev[3].record(); torch.cuda.synchronize()
    ms_fit = ev[0].elapsed_time(ev[1]) / reps
    ms_comm = ev[2].elapsed_time(ev[3]) / reps
    stats = torch.tensor([ms_fit, ms_comm, float(solver.n_halo), float(solver.n_own - solver.n_int), float(solver.send_idx.numel())],
                         dtype=torch.float64, device=(dev if dist is None or dist.get_backend() == "nccl" else "cpu"))
    if dist is not None:
        dist.all_reduce(stats, op=dist.ReduceOp.MAX)
    ms_fit, ms_comm, halo_max, bnd_max, send_max = stats.tolist()
    B_fit = bytes_per_fit_indexed(dim, order, nk)
    achieved = B_fit * solver.n_own / (ms_fit * 1e-3) / 1e9
    out = {"metric": "local fits/s (whole node)", "value": N * a.steps / dt, "unit": "fits/s",
           "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": dt / a.steps * 1e3,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
           "config": {"workload": "C5 sharded (BASELINE configs[4] literal): one Morton-ordered 3D Halton cloud of %d points, %d per "
                                  "rank, 40 neighbours, order 2, WEIGHT_CENTER; own-points-only neighbour search + halo band, "
                                  "index-based fit from local tables, halo values exchanged per step (all_to_all_single) under the "
                                  "interior fits, explicit field update" % (N, n_local),
                      "fits_per_gpu": n_local, "bytes_per_fit": B_fit},
           "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBPS,
                        "traffic": None, "traffic_source": None, "kernel_ms": ms_fit, "kernel": kernel,
                        "gathered_bytes_per_fit": 8 * nk * (dim + 1),
                        "gather_rate_GBps": 8 * nk * (dim + 1) * solver.n_own / (ms_fit * 1e-3) / 1e9,
                        "note": "index-based bytes (4 nk + 8 (dim+1) + 8 no + 20 per fit): never mixed with the dense-layout metric, and "
                                "not an HBM-bound kernel — the 8 nk (dim+1) bytes per fit of neighbour rows are gathered from the local "
                                "tables through L2 (gather_rate_GBps); kernel_ms = interior + boundary launch of a step"},
           "sharded": {"points": N, "ms_fit": ms_fit, "ms_comm_alone": ms_comm, "ms_step": dt / a.steps * 1e3,
                       "halo_points_max_over_ranks": int(halo_max), "boundary_cases_max_over_ranks": int(bnd_max),
                       "sent_values_max_over_ranks": int(send_max), "halo_bytes_received_per_step": int(halo_max) * 8,
                       "full_allgather_bytes_per_step": 8 * (N - n_local), "halo_radius": solver.halo_radius,
                       "band_points_received_in_setup": int(getattr(solver, "band_points_received", 0)),
                       "overlap_efficiency": ms_fit / (dt / a.steps * 1e3), "setup_s": t_setup}}
    if parity:
        solver.exchange_begin(); solver.exchange_end()          # a collective: every rank takes part; rank 0 then checks its shard
        torch.cuda.synchronize()
    if parity and rank == 0:
        # first 1 024 local cases against the oracle on the same (dense-gathered) inputs of the CURRENT field
        from oracle import oracle
        import _parity
        ns = min(solver.n_own, 1024)
        h = solver.hoods32[:ns].long()
        xk_h = solver.S_tab[h].cpu().numpy(); fk_h = solver.values[h].cpu().numpy(); xi_h = solver.S_tab[:ns].cpu().numpy()
        fi_d = torch.zeros((ns, no), dtype=torch.float64, device=dev); fi_d[:, 0] = solver.values[:ns]
        fi_in = fi_d.cpu().numpy()
        whip.fit_cloud_device(dim, order, solver.S_tab, solver.values, solver.hoods32[:ns], fi_d, solver.nk_t[:ns], solver.kn_t[:ns],
                              solver.wm_t[:ns], point_index=solver.pidx[:ns])
        torch.cuda.synchronize()
        meta = (np.full(ns, nk, np.int32), np.full(ns, order, np.int32), np.full(ns, cfg["knowns"], np.int64), np.full(ns, cfg["wm"], np.int32))
        fi_o = fi_in.copy()
        oracle.fit_many(dim, xk_h, fk_h, meta[0], xi_h, fi_o, None, 0, meta[1], meta[2], meta[3], ntasks=8)
        truth = _parity.truth_fit(dim, xk_h, fk_h, meta[0], xi_h, fi_in, meta[1], meta[2], meta[3])
        acc = _parity.accounting(fi_d.cpu().numpy(), fi_o, truth=truth)
        acc["reference"] = "CPU oracle on the first %d local cases, current field" % ns
        out["parity"] = {"vs_oracle": acc}
    if outputs:
        out["_outputs"] = outputs
    return out


def cpu_baseline(oracle, cfg, xk_d, fk_d, xi_d, F, n, no):
    """The CPU oracle (a restatement of the reference's Cython/OpenMP/LAPACK path, kind "port") timed on this
    box's host cores on a bounded sample of the same workload."""
    dim, order, nk = cfg["dim"], cfg["order"], cfg["nk"]
    cores = len(os.sched_getaffinity(0))
    ns = min(n, 400_000)
    xk_h = xk_d[:ns].cpu().numpy(); fk_h = fk_d[:ns].cpu().numpy(); xi_h = xi_d[:ns].cpu().numpy()
    meta = (np.full(ns, nk, np.int32), np.full(ns, order, np.int32), np.full(ns, cfg["knowns"], np.int64),
            np.full(ns, cfg["wm"], np.int32))

    def rate(threads, budget_s):
        best, reps, t_all = 0.0, 0, time.perf_counter()
        while True:
            fi = np.zeros((ns, no)); fi[:, 0] = F[:ns]
            t0 = time.perf_counter()
            oracle.fit_many(dim, xk_h, fk_h, meta[0], xi_h, fi, None, 0, meta[1], meta[2], meta[3], ntasks=threads)
            dt = time.perf_counter() - t0
            best = max(best, ns / dt); reps += 1
            if (reps >= 3 and time.perf_counter() - t_all > budget_s) or reps >= 20:
                return best, reps
    # The restated algorithm keeps the reference's four malloc/free per case (lapackdrivers.pyx:557-560), which stops scaling
    # long before a 256-thread host is full: time a ladder of team sizes and report the best one as the baseline.
    ladder = sorted({t for t in (8, 16, 32, 64, 128, cores) if t <= cores})
    rates = {}
    for t in ladder:
        rates[t], _ = rate(t, 2.5)
    best_t = max(rates, key=rates.get)
    return {"value": rates[best_t], "unit": "fits/s", "cores": best_t, "kind": "port",
            "sample": "%d cases of the same workload, best pass per team size, OpenMP static schedule; team sizes tried: %s "
                      "(host has %d hardware threads)" % (ns, ", ".join("%d: %.3g" % (t, rates[t]) for t in ladder), cores),
            "value_8_threads": rates.get(8, rates[ladder[0]]), "value_all_threads": rates[cores]}


def headline_line(res, world, a, dt, units):
    out = {"metric": "local fits/s (whole node)", "value": world * units * a.steps / dt, "unit": "fits/s",
           "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": dt / a.steps * 1e3,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
           "config": {k: res[k] for k in ("workload", "fits_per_gpu", "bytes_per_fit") if k in res},
           "roofline": res["roofline"]}
    for k in ("nrhs", "prepare_ms_device_arrays", "prepare_operator_ms", "value_including_prepare", "time_stepping", "parity"):
        if k in res:
            out[k] = res[k]
    return out


def _sig(x, nd=4):
    """x rounded to nd significant digits (compact line only)."""
    if x is None or isinstance(x, (str, bool, int)):
        return x
    try:
        return float("%.*g" % (nd, float(x)))
    except (TypeError, ValueError):
        return x


COMPACT_LIMIT = 1750        # bytes: the driver keeps a 2 KB tail of stdout and parses its last line


def compact_line(full, full_path=None):
    """The LAST stdout line: the contract's fields + roofline + cpu_baseline + a parity digest + ONE [ms_per_step, frac] pair
    per side config, guaranteed under COMPACT_LIMIT bytes (fields are dropped from the end of `optional` until it fits).
    Everything else (per-config roofline / parity blocks, cond histograms) is in the full record: an earlier stdout line
    prefixed '# full: ' and, when writable, gpurun_out/bench_full.json."""
    out = {k: full.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                    "scaling", "vs_baseline", "dtype", "data")}
    for k in ("value", "ms_per_step"):
        out[k] = _sig(out[k], 6)
    cfg = full.get("config", {})
    out["config"] = {"workload": str(cfg.get("workload", ""))[:200], "fits_per_gpu": cfg.get("fits_per_gpu"),
                     "bytes_per_fit": _sig(cfg.get("bytes_per_fit"), 6)}
    r = full.get("roofline", {})
    out["roofline"] = {"bound": r.get("bound"), "achieved": _sig(r.get("achieved"), 5), "peak": r.get("peak"), "unit": r.get("unit"),
                       "frac": _sig(r.get("frac")), "traffic": _sig(r.get("traffic"), 5), "traffic_source": r.get("traffic_source"),
                       "kernel_ms": _sig(r.get("kernel_ms"), 5), "kernel": r.get("kernel")}
    c = full.get("cpu_baseline")
    if c:
        out["cpu_baseline"] = {"value": _sig(c.get("value")), "unit": c.get("unit"), "cores": c.get("cores"), "kind": c.get("kind"),
                               "sample": str(c.get("sample", ""))[:60], "value_8_threads": _sig(c.get("value_8_threads"))}
    optional = []
    p = full.get("parity", {})
    g = p.get("vs_reference_golden") or p.get("vs_oracle")
    if g:
        d = {"E_max": _sig(g.get("E_max"), 3), "N_max": _sig(g.get("N_max"), 3), "strict_columns": g.get("strict_1e-10_columns"),
             "columns": g.get("columns"), "golden": g.get("golden") or "oracle"}
        s = p.get("strict_mode")
        if s:
            d["strict_mode"] = {"E_max": _sig(s.get("E_max"), 3), "strict_columns": s.get("strict_1e-10_columns"),
                                "ms_per_step": _sig(s.get("ms_per_step"), 4)}
        a = p.get("accurate_mode")
        if a:
            d["accurate_mode"] = {"E_max": _sig(a.get("E_max"), 3), "strict_columns": a.get("strict_1e-10_columns"),
                                  "ms_per_step": _sig(a.get("ms_per_step"), 4), "frac": _sig(a.get("frac"), 3)}
        optional.append(("parity", d))
    keep = {"sharded": ("points", "points_per_rank", "fits_per_s", "ms_step", "ms_fit", "ms_comm_alone", "overlap_efficiency",
                        "halo_points_max_over_ranks", "halo_bytes_received_per_step", "full_allgather_bytes_per_step"),
            "rccl": ("world_size", "backend", "allreduce_sum_ok")}
    for k in ("sharded", "rccl"):
        if k in full and isinstance(full[k], dict):
            optional.append((k, {kk: _sig(full[k][kk], 5) for kk in keep[k] if kk in full[k]}))
    side = full.get("configs")
    if side:
        summ = {}
        for k, v in side.items():
            if "error" in v:
                summ[k] = "error"
            else:
                summ[k] = [_sig(v.get("ms_per_step")), _sig(v.get("roofline", {}).get("frac"), 3)]
                if v.get("roofline", {}).get("valu_frac") is not None:       # [ms, fraction of the HBM peak, fraction of the fp64 vector peak]
                    summ[k].append(_sig(v["roofline"]["valu_frac"], 3))
        optional.append(("configs_summary", summ))
    if full_path:
        optional.append(("full", full_path))
    for k, v in optional:
        out[k] = v
    drop = [k for k, _ in optional][::-1]
    size = lambda: len(json.dumps(out, separators=(",", ":")))
    while size() > COMPACT_LIMIT and isinstance(out.get("configs_summary"), dict) and len(out["configs_summary"]) > 6:
        out["configs_summary"].popitem()                              # the newest side lines go first; the BASELINE configs lead the dict
    while size() > COMPACT_LIMIT and drop:
        out.pop(drop.pop(0), None)
    return out


def emit(full):
    """Rank 0's output: the full record on an EARLIER line (not parseable as the headline: prefixed), then the compact headline
    as the last line of stdout."""
    path = None
    try:
        d = os.path.join(ROOT, "gpurun_out")
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, "bench_full.json")
        with open(path, "w") as f:
            json.dump(full, f)
        path = "gpurun_out/bench_full.json"
    except OSError:
        path = None
    print("# full: " + json.dumps(full), flush=True)
    print(json.dumps(compact_line(full, path), separators=(",", ":")), flush=True)


def measure_cloud(name, cfg, n, dev, timer, steps, warmup, rank):
    """One BASELINE shape through the INDEX-BASED device API (wlsqm.hip.fit_cloud_device: point tables S, F + int32 neighbour lists;
    the kernels gather the rows themselves), points ordered along a Morton curve so that the gathers of a tile stay in L2.
    Reported with the index-based bytes (never mixed with the dense-layout metric) plus the rate of the gathered rows."""
    import torch
    import wlsqm.hip as whip
    dim, order, nk = cfg["dim"], cfg["order"], cfg["nk"]
    no = NDOF[dim][order]
    S, F, hoods = build_problem(cfg, n, rank, device=dev)
    S_d = torch.from_numpy(np.ascontiguousarray(S)).to(dev)
    perm = morton_order_device(S_d)
    inv = torch.empty_like(perm); inv[perm] = torch.arange(n, device=dev, dtype=perm.dtype)
    S_d = S_d[perm].contiguous()
    F_d = torch.from_numpy(F).to(dev)[perm].contiguous()
    h_d = inv[torch.from_numpy(hoods).to(dev)[perm].long()].to(torch.int32).contiguous()
    del perm, inv
    nk_d = torch.full((n,), nk, dtype=torch.int32, device=dev)
    kn_d = torch.full((n,), cfg["knowns"], dtype=torch.int64, device=dev)
    wm_d = torch.full((n,), cfg["wm"], dtype=torch.int32, device=dev)
    fi_d = torch.zeros((n, no), dtype=torch.float64, device=dev); fi_d[:, 0] = F_d
    args = (dim, order, S_d, F_d, h_d, fi_d, nk_d, kn_d, wm_d)
    dt = timer.run(lambda: whip.fit_cloud_device(*args), steps, warmup)
    kernel = whip.last_kernel()
    ms_kernel = whip.time_fit_cloud_device(*args, reps=min(max(steps, 20), 200))
    B_fit = bytes_per_fit_indexed(dim, order, nk)
    achieved = B_fit * n / (ms_kernel * 1e-3) / 1e9
    res = {"workload": "%s index-based: %s; %d local fits per GPU per step from device-resident point tables (Morton order) + int32 "
                       "neighbour lists" % (name, cfg["desc"], n),
           "fits_per_gpu": n, "bytes_per_fit": B_fit, "ms_per_step": dt / steps * 1e3, "fits_per_s": n * steps / dt,
           "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBPS,
                        "traffic": None, "traffic_source": None, "kernel_ms": ms_kernel, "kernel": kernel,
                        "gathered_bytes_per_fit": 8 * nk * (dim + 1),
                        "gather_rate_GBps": 8 * nk * (dim + 1) * n / (ms_kernel * 1e-3) / 1e9,
                        "note": "index-based bytes (4 nk + 8 (dim+1) + 8 no + 20 per fit): not an HBM-bound kernel — the 8 nk (dim+1) "
                                "bytes per fit of neighbour rows are gathered from the point tables through L2 (gather_rate_GBps)"}}
    if rank == 0:
        # the same cases as dense rows through the dense kernel of the shape: the gathering kernel is the dense one behind its fetch
        m = min(n, 4096)
        hh = h_d[:m].long()
        fa = torch.zeros((m, no), dtype=torch.float64, device=dev); fa[:, 0] = F_d[:m]
        fb = fa.clone()
        whip.fit_cloud_device(dim, order, S_d, F_d, h_d[:m], fa, nk_d[:m], kn_d[:m], wm_d[:m])
        whip.fit_many_device(dim, order, S_d[hh].contiguous(), F_d[hh].contiguous(), nk_d[:m], S_d[:m].contiguous(), fb, kn_d[:m], wm_d[:m])
        torch.cuda.synchronize()
        res["parity"] = {"vs_dense_kernel": {"cases": m, "dense_kernel": whip.last_kernel(), "bit_identical": bool(torch.equal(fa, fb)),
                                             "max_abs_diff": float((fa - fb).abs().max())}}
    return res, dt


def side_configs(a, dev, timer, rank, parity):
    """Every other BASELINE config with the same --steps / --warmup (single GPU).  Each entry carries its own roofline block."""
    import copy
    import torch
    side = {}
    short = dict(steps=max(1, min(a.steps, 20)), warmup=min(a.warmup, 3))

    only = [s for s in os.environ.get("WLSQM_BENCH_SIDE", "").split(",") if s]      # (experiments: only the side lines whose key contains one of these)

    def add(key, fn):
        if only and not any(s in key for s in only):
            return
        t0 = time.perf_counter()
        try:
            res = fn()
            res = res[0] if isinstance(res, tuple) else res
            res["wall_s_including_setup"] = time.perf_counter() - t0
            side[key] = res
        except Exception as e:      # a side config must never take the headline down with it
            side[key] = {"error": "%s: %s" % (type(e).__name__, e)}
        torch.cuda.empty_cache()

    add("C1@10k", lambda: measure_fit("C1", CONFIGS["C1"], 10_000, dev, timer, a.steps, a.warmup, rank, parity))
    add("C1@4M", lambda: measure_fit("C1", CONFIGS["C1"], 4_000_000, dev, timer, a.steps, a.warmup, rank, False))
    add("C3@1M", lambda: measure_fit("C3", CONFIGS["C3"], 1_000_000, dev, timer, a.steps, a.warmup, rank, parity))
    add("C4@1M,R=%d" % (a.nrhs or 256), lambda: measure_c4(CONFIGS["C4"], 1_000_000, a.nrhs or 256, dev, timer, short["steps"],
                                                           short["warmup"], rank, parity))
    add("C5@1M", lambda: measure_fit("C5", CONFIGS["C5"], 1_000_000, dev, timer, a.steps, a.warmup, rank, parity))
    add("C5@16M", lambda: measure_fit("C5", CONFIGS["C5"], 16_000_000, dev, timer, short["steps"], short["warmup"], rank, False))
    # the same functions with their flags (do_sens, the *_iterative_* entry points): not BASELINE configs, driver-timed all the same
    for cname, cn in (("C2", 1_000_000), ("C3", 400_000), ("C5", 1_000_000)):
        for ex in ("sens", "iter"):
            add("%s+%s@%s" % (cname, ex, "1M" if cn == 1_000_000 else "400k"),
                lambda cname=cname, cn=cn, ex=ex: measure_fit(cname, CONFIGS[cname], cn, dev, timer, short["steps"], short["warmup"], rank, parity and ex == "iter", extras=ex))

    def sharded():
        b = copy.copy(a)
        b.ncases, b.steps, b.warmup = 2_000_000, short["steps"], short["warmup"]
        line = run_sharded(b, dev, None, rank, 1, timer, parity)
        return {k: line[k] for k in ("config", "steps", "ms_per_step", "value", "roofline", "sharded", "parity") if k in line}
    add("C5-sharded@2M-per-rank", sharded)
    # index-based input of configs[2]'s shape (the gathering form of the staged kernel); last, so that the order of the earlier entries is the one
    # of the earlier rounds' records
    add("C3-indexed@1M", lambda: measure_cloud("C3", CONFIGS["C3"], 1_000_000, dev, timer, short["steps"], short["warmup"], rank))
    if only:        # (experiments only — WLSQM_BENCH_SIDE=indexed: the other two BASELINE shapes through the gathering kernels)
        for cname in ("C2", "C5"):
            add("%s-indexed@1M" % cname, lambda cname=cname: measure_cloud(cname, CONFIGS[cname], 1_000_000, dev, timer, short["steps"], short["warmup"], rank))
    # 3D orders 3 and 4 (20 / 35 unknowns; round 4: the staged kernel with LDS rows / moments + the four-lanes-per-case solve), with a
    # sample of the batch checked against the CPU port as in the sharded line (no reference golden at these shapes)
    # neighbour lists that are NOT sorted by distance: the BASELINE shapes with every row shuffled, and the shape of
    # the reference's own harness (ball query, ragged counts, order 4, F known)
    for cname in ("C2", "C3", "C5"):
        add("%s-unsorted@1M" % cname, lambda cname=cname: measure_extra_shape(cname + "-unsorted", CONFIGS[cname], 1_000_000, dev, timer,
                                                                             short["steps"], short["warmup"], rank, parity, unsorted=True))
    add("C3-ball@400k", lambda: measure_ball("C3-ball", 400_000, dev, timer, short["steps"], short["warmup"], rank, parity))
    add("C3-ball-nkorder@400k", lambda: measure_ball("C3-ball-nkorder", 400_000, dev, timer, short["steps"], short["warmup"], rank, parity, nk_order=True))
    # the ACCURATE mode beyond the headline's parity block: configs[4]'s shape, the reference's default mask, shuffled rows
    add("C5-accurate@1M", lambda: measure_fit("C5-accurate", CONFIGS["C5"], 1_000_000, dev, timer, short["steps"], short["warmup"], rank, parity, extras="accurate"))
    add("C2-accurate-Fknown@1M", lambda: measure_fit("C2-accurate-Fknown", dict(CONFIGS["C2"], knowns=1, desc=CONFIGS["C2"]["desc"] + " [F known: simple.pyx:60-61]"),
                                                       1_000_000, dev, timer, short["steps"], short["warmup"], rank, parity, extras="accurate"))
    add("C2-accurate-unsorted@1M", lambda: measure_fit("C2-accurate-unsorted", CONFIGS["C2"], 1_000_000, dev, timer, short["steps"], short["warmup"], rank,
                                                         parity, extras="accurate", unsorted=True))
    # (3Do4-64nb: 40 neighbours for 35 unknowns is a nearly determined fit — its parity block is mostly conditioning noise; 64 is the workload
    # a user of that order would run)
    for key, order, cn, knb in (("3Do3@1M", 3, 1_000_000, 40), ("3Do4@400k", 4, 400_000, 40), ("3Do4-64nb@200k", 4, 200_000, 64)):
        cfg = dict(CONFIGS["C5"], order=order, nk=knb, desc="3D order-%d, Halton, %d neighbours, WEIGHT_CENTER, all DOFs unknown" % (order, knb))
        add(key, lambda key=key, cfg=cfg, cn=cn: measure_extra_shape(key, cfg, cn, dev, timer, short["steps"], short["warmup"], rank, parity))
    return side


def measure_ball(name, n, dev, timer, steps, warmup, rank, parity, order=4, max_nk=100, mean_nk=64, nk_order=False):
    """The shape of the reference's own harness (examples/wlsqm_example.py:103-133: `cKDTree.query_ball_point`, order 4, knowns = F,
    max_nk = 100): every point's neighbours are ALL points within a radius — a ragged count per case, in NO particular order (the
    tree's), padded to max_nk slots.  Radius chosen for ~mean_nk neighbours on n Halton points; the GPU ball search returns them
    nearest first, so every row's valid entries are shuffled to look like the reference's input.  Dense device-resident rows."""
    import math
    import torch
    import wlsqm.hip as whip
    dim, no = 2, NDOF[2][order]
    S = synth.halton(n, dim, skip=1 + rank * n); F = synth.field(S)
    S_d = torch.from_numpy(np.ascontiguousarray(S)).to(dev); F_d = torch.from_numpy(F).to(dev)
    radius = math.sqrt(mean_nk / (math.pi * n))
    h_d, nk_d = whip.ball(S_d, radius, max_nk)
    g = torch.Generator(device=dev); g.manual_seed(7 + rank)
    keys = torch.rand((n, max_nk), device=dev, generator=g)
    keys[torch.arange(max_nk, device=dev)[None, :] >= nk_d[:, None]] = 2.0          # padding stays behind the valid entries
    h_d = torch.gather(h_d, 1, torch.argsort(keys, dim=1)).contiguous()
    del keys
    cases = torch.arange(n, device=dev)
    if nk_order:
        # the CASES in neighbour-count order (what the host entry points do themselves while they stage a ragged batch, csrc/api.hip; a caller
        # of the device-resident API lays its rows out as it likes): a wave's 64 cases then need the same chunks
        cases = torch.argsort(nk_d, stable=True)
        h_d = h_d[cases].contiguous(); nk_d = nk_d[cases].contiguous()
    hh = h_d.long()
    xk_d = S_d[hh].contiguous(); fk_d = F_d[hh].contiguous()
    del hh
    xi_d = S_d[cases].contiguous()
    fi_d = torch.zeros((n, no), dtype=torch.float64, device=dev); fi_d[:, 0] = F_d[cases]
    kn_d = torch.ones((n,), dtype=torch.int64, device=dev)
    wm_d = torch.full((n,), 2, dtype=torch.int32, device=dev)
    args = (dim, order, xk_d, fk_d, nk_d, xi_d, fi_d, kn_d, wm_d)
    # (device-resident counts: the caller says that its rows are ragged — wlsqm.hip.row_hint; the host entry points see it themselves)
    with whip.row_hint("ragged", sorted=False):
        dt = timer.run(lambda: whip.fit_many_device(*args), steps, warmup)
        kernel = whip.last_kernel()
        ms_kernel = whip.time_fit_device(*args, reps=min(max(steps, 10), 100))
    nk_mean = float(nk_d.double().mean()); nk_min = int(nk_d.min()); nk_max = int(nk_d.max())
    B_fit = 8.0 * nk_mean * (dim + 1) + 8 * dim + 8 * no + 8 + 20          # SURVEY section 8d with the cases' own neighbour counts
    achieved = B_fit * n / (ms_kernel * 1e-3) / 1e9
    res = {"workload": "%s: 2D order-%d, %d Halton points, ball query r = %.5f (nk %d..%d, mean %.1f, %d slots), neighbours UNSORTED, "
                       "WEIGHT_CENTER, F known; device-resident dense xk/fk" % (name, order, n, radius, nk_min, nk_max, nk_mean, max_nk),
           "fits_per_gpu": n, "bytes_per_fit": B_fit, "ms_per_step": dt / steps * 1e3, "fits_per_s": n * steps / dt,
           "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBPS,
                        "traffic": None, "kernel_ms": ms_kernel, "kernel": kernel, "algorithmic_bytes_per_launch": B_fit * n,
                        "note": "algorithmic bytes count the valid neighbours only; the rows are padded to %d slots" % max_nk}}
    if parity and rank == 0:
        from oracle import oracle
        sel = torch.nonzero(nk_d >= no + 8)[:, 0]                          # (nearly determined neighbourhoods are noise, not signal)
        if nk_order and sel.numel() > 1024:
            sel = sel[torch.linspace(0, sel.numel() - 1, 1024, device=dev).long()]      # (every neighbour count, not the smallest only)
        sel = sel[:1024]
        m = int(sel.numel())
        xk, fk, xi = (t[sel].cpu().numpy() for t in (xk_d, fk_d, xi_d))
        got = fi_d[sel].cpu().numpy()
        ref = np.zeros((m, no)); ref[:, 0] = F_d[cases[sel]].cpu().numpy()
        oracle.fit_many(dim, xk, fk, nk_d[sel].cpu().numpy(), xi, ref, None, 0, np.full(m, order, np.int32), np.ones(m, np.int64),
                        np.full(m, 2, np.int32), ntasks=8)
        scale = np.abs(ref).max(axis=0)
        E = np.abs(got - ref).max(axis=0) / np.where(scale > 0, scale, 1.0)
        res["parity"] = {"vs_oracle": {"cases": m, "E_max": float(E.max()), "columns": int(no), "columns_le_1e-8": int((E <= 1e-8).sum())}}
    return res, dt


def measure_extra_shape(name, cfg, n, dev, timer, steps, warmup, rank, parity, unsorted=False):
    """measure_fit for a shape outside BASELINE's configs; the first 1 024 cases of the batch against the CPU port (checker only)."""
    res, dt = measure_fit(name, cfg, n, dev, timer, steps, warmup, rank, False, keep=True, unsorted=unsorted)
    t = res.pop("_tensors")
    if parity and rank == 0:
        from oracle import oracle
        m = 1024
        dim, order, no = cfg["dim"], cfg["order"], NDOF[cfg["dim"]][cfg["order"]]
        xk, fk, xi = (t[k][:m].cpu().numpy() for k in ("xk", "fk", "xi"))
        got = t["fi"][:m].cpu().numpy()
        ref = np.zeros((m, no)); ref[:, 0] = t["F"][:m]
        oracle.fit_many(dim, xk, fk, np.full(m, cfg["nk"], np.int32), xi, ref, None, 0, np.full(m, order, np.int32),
                        np.full(m, cfg["knowns"], np.int64), np.full(m, cfg["wm"], np.int32), ntasks=8)
        scale = np.abs(ref).max(axis=0)
        E = np.abs(got - ref).max(axis=0) / np.where(scale > 0, scale, 1.0)
        res["parity"] = {"vs_oracle": {"cases": m, "E_max": float(E.max()), "columns": int(no), "columns_le_1e-8": int((E <= 1e-8).sum()),
                                       "note": "column metric max_j |fi - fi_oracle| / max_j |fi_oracle| on the first 1 024 cases; fast mode "
                                               "(moment form, unpivoted LDL^T) against the port's Ruiz-scaled pivoted LU"}}
    del t
    return res, dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--config", default=None, choices=sorted(CONFIGS),
                    help="measure this config as `value` (default: C2 as `value`, with --full plus every other config under `configs`)")
    ap.add_argument("--ncases", type=int, default=None, help="local fits per GPU per step (default 1M; --sharded: 2M points per rank)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline: parity, CPU baseline, dedicated kernel timings, the "
                         "numerics modes, the side configs (single GPU) or the sharded configs[4] block (N > 1), and the full record")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned as DIR/<name>.npy (float64, <= 64 MB in all)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip the CPU baseline")
    ap.add_argument("--no-parity", action="store_true", help="(--full) skip the parity checks (profiling passes)")
    ap.add_argument("--no-side-configs", action="store_true", help="(--full) C2 only")
    ap.add_argument("--nrhs", type=int, default=None, help="C4: right-hand sides stacked per step (default 256 = BASELINE configs[3])")
    ap.add_argument("--sharded", action="store_true",
                    help="C5 in the literal form of BASELINE configs[4]: one Morton-ordered cloud of --ncases points PER RANK, "
                         "index-based fit, time-stepped with a halo exchange between ranks (wlsqm/sharded.py)")
    a = ap.parse_args()
    if a.ncases is None:
        a.ncases = 2_000_000 if a.sharded else 1_000_000

    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if a.gpus > 1 and world != a.gpus:
        raise SystemExit("bench.py --gpus %d must be launched with torch.distributed.run --nproc-per-node %d" % (a.gpus, a.gpus))
    # REHEARSAL ONLY (never the driver's path): WLSQM_BENCH_REHEARSAL=1 runs the N > 1 flow with all ranks on GPU 0 over gloo, to
    # exercise the multi-rank control flow on a one-GPU box (RCCL needs one GPU per rank); the line is marked "rehearsal"
    rehearsal = os.environ.get("WLSQM_BENCH_REHEARSAL") == "1"
    if rehearsal:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if "RANK" in os.environ:        # launched by torch.distributed.run: one rank per GPU, RCCL ("nccl") process group
        import torch.distributed as dist
        if rehearsal:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)
    timer = Timer(dist, dev)
    headline = a.config or "C2"
    cfg = CONFIGS[headline]
    parity = a.full and not a.no_parity
    dump = a.dump_outputs is not None and rank == 0

    if a.sharded:
        out = run_sharded(a, dev, dist, rank, world, timer, parity, dump=dump)
        outputs = out.pop("_outputs", None)
    elif headline == "C4":
        R = a.nrhs or 256
        res, dt = measure_c4(cfg, a.ncases, R, dev, timer, a.steps, a.warmup, rank, parity, full=a.full, dump=dump)
        outputs = res.pop("_outputs", None)
        out = headline_line(res, world, a, dt, a.ncases * R)
    else:
        res, dt = measure_fit(headline, cfg, a.ncases, dev, timer, a.steps, a.warmup, rank, parity, keep=True, full=a.full, dump=dump)
        outputs = res.pop("_outputs", None)
        tensors = res.pop("_tensors")
        out = headline_line(res, world, a, dt, a.ncases)
        if a.full and rank == 0 and world == 1 and not a.no_cpu_baseline:
            from oracle import oracle
            out["cpu_baseline"] = cpu_baseline(oracle, cfg, tensors["xk"], tensors["fk"], tensors["xi"], tensors["F"], a.ncases,
                                               NDOF[cfg["dim"]][cfg["order"]])
        del tensors
        torch.cuda.empty_cache()
        if a.full and a.config is None and world == 1 and not a.no_side_configs:
            out["configs"] = side_configs(a, dev, timer, rank, parity)
        if a.full and a.config is None and world > 1 and not a.no_side_configs:
            # BASELINE configs[4] in its literal form, in the driver's own scaling run: ONE 16M-point 3D cloud partitioned over the
            # N ranks, halo values exchanged over RCCL every step (wlsqm/sharded.py).  Reported beside the C2 weak-scaling value.
            import copy
            b = copy.copy(a)
            b.ncases, b.steps, b.warmup = 16_000_000 // world, max(1, min(a.steps, 20)), min(a.warmup, 3)
            chk = torch.full((1 << 16,), float(rank + 1), dtype=torch.float64, device=("cpu" if rehearsal else dev))
            dist.all_reduce(chk)
            line = run_sharded(b, dev, dist, rank, world, timer, parity)
            sh = dict(line["sharded"])
            sh.update({"fits_per_s": line["value"], "points_per_rank": b.ncases, "steps": b.steps,
                       "kernel": line["roofline"]["kernel"], "gather_rate_GBps": line["roofline"]["gather_rate_GBps"]})
            out["sharded"] = sh
            out["rccl"] = {"world_size": world, "backend": dist.get_backend(),
                           "allreduce_sum_ok": bool((chk == world * (world + 1) / 2).all().item())}
            if "parity" in line:
                out["sharded_parity"] = line["parity"]
    if rehearsal:
        out["rehearsal"] = "all ranks on GPU 0, gloo: control-flow check only, not a measurement"
    if outputs:
        dump_outputs(a.dump_outputs, outputs)
    if rank == 0:
        if a.full:
            emit(out)
        else:
            print(json.dumps(compact_line(out), separators=(",", ":")), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
