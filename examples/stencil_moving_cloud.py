#!/usr/bin/env python3
"""A cloud whose points move while its neighbour lists stay (a Lagrangian step): the points are advected by a rotating velocity field,
and every step refreshes the gradient and Laplacian stencils in place (wlsqm.hip.StencilOperator.update: one fused kernel, no
allocation, no synchronisation) and applies them to the field the points carry.  Runs eager and as one HIP graph replay per step
(update + apply captured once, the points moved with copy_), and prints its agreement with an operator built afresh on the last
positions and with fit_cloud_device there."""
import os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "python-wlsqm_amd"))
import wlsqm
import wlsqm.hip

n, nk, order, steps, dt = 200_000, 32, 2, 20, 2e-4
rng = np.random.default_rng(1)
dev = torch.device("cuda", 0)
S0 = torch.from_numpy(rng.uniform(0.0, 1.0, (n, 2))).to(dev)
hoods = wlsqm.hip.knn(S0, nk)                                       # searched once: the steps below are far too short to reorder neighbours
nk_d = torch.full((n,), nk, dtype=torch.int32, device=dev)
knowns = torch.full((n,), wlsqm.b2_F, dtype=torch.int64, device=dev)
wm = torch.full((n,), wlsqm.WEIGHT_CENTER, dtype=torch.int32, device=dev)
rows = wlsqm.hip.stencil_rows(2, order, "gradient", "laplacian", device=dev)

S = S0.clone()
t0 = time.perf_counter()
op = wlsqm.hip.StencilOperator(2, order, S, hoods, nk_d, knowns, wm, rows)      # keeps hoods, nk_d, knowns, wm and rows for update()
torch.cuda.synchronize()
print("gradient + Laplacian on %d points: built in %.1f ms, %.1f MB" % (n, (time.perf_counter() - t0) * 1e3, op.memory_used() / 1e6))

f = torch.sin(3.0 * S0[:, 0]) * torch.cos(2.0 * S0[:, 1])           # carried by the points: constant along their paths
out = torch.empty((3, n), dtype=torch.float64, device=dev)


def move(P):
    """One forward-Euler step of the rigid rotation about (0.5, 0.5)."""
    return P + dt * torch.stack([-(P[:, 1] - 0.5), P[:, 0] - 0.5], dim=1)


def refresh():
    op.update(S, check=False)                                       # the stencils where the points are now
    op.apply(f, out=out)                                            # d/dx, d/dy and the Laplacian of the carried field


refresh()                                                           # warm-up outside the capture
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(steps):
    S.copy_(move(S))
    refresh()
torch.cuda.synchronize(); t_eager = (time.perf_counter() - t0) / steps
eager, S_end = out.clone(), S.clone()

S.copy_(S0)
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
    refresh()
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(steps):
    S.copy_(move(S))
    graph.replay()
torch.cuda.synchronize(); t_graph = (time.perf_counter() - t0) / steps

fresh = wlsqm.hip.StencilOperator(2, order, S_end, hoods, nk_d, knowns, wm, rows)
want = fresh.apply(f)
fi = torch.zeros((n, wlsqm.number_of_dofs(2, order)), dtype=torch.float64, device=dev)
fi[:, 0] = f
wlsqm.hip.fit_cloud_device(2, order, S_end, f, hoods, fi, nk_d, knowns, wm)
fit = torch.stack([fi[:, wlsqm.i2_X], fi[:, wlsqm.i2_Y], fi[:, wlsqm.i2_X2] + fi[:, wlsqm.i2_Y2]])
print("%d steps of move + update + apply: eager %.3f ms per step, one HIP graph replay per step %.3f ms (identical: %s)"
      % (steps, t_eager * 1e3, t_graph * 1e3, bool(torch.equal(out, eager))))
print("against an operator built afresh on the last positions: identical %s; against fit_cloud_device there: max |difference| %.2e "
      "of max |value| %.2e" % (bool(torch.equal(eager, want)), float((eager - fit).abs().max()), float(fit.abs().max())))
