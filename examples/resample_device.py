#!/usr/bin/env python3
"""Fit on a cloud, resample value and gradient to a grid, every time step, inside ONE HIP graph: an interpolation plan searches the
grid points' models once; after that a step is gather + fit + evaluate with nothing crossing PCIe and no host synchronisation."""
import os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "python-wlsqm_amd"))
import wlsqm
import wlsqm.hip

n, nk, order, side = 200_000, 32, 2, 512
rng = np.random.default_rng(1)
dev = torch.device("cuda", 0)
S_d = torch.from_numpy(rng.uniform(0.0, 1.0, (n, 2))).to(dev)
h_d = wlsqm.hip.knn(S_d, nk).long()
solver = wlsqm.ExpertSolver(dimension=2, nk=np.full(n, nk, np.int32), order=np.full(n, order, np.int32),
                            knowns=np.full(n, wlsqm.b2_F, np.int64), weighting_method=np.full(n, wlsqm.WEIGHT_CENTER, np.int32))
solver.prepare_device(S_d, S_d[h_d].contiguous())

# the resampling grid: a plan per mode, built once (nearest: the model of the nearest origin; continuous: the weighted average of the
# models within r, about 12 of them here)
ax = torch.linspace(0.05, 0.95, side, dtype=torch.float64, device=dev)
G_d = torch.stack(torch.meshgrid(ax, ax, indexing="ij"), dim=-1).reshape(-1, 2)
torch.cuda.synchronize(); t0 = time.perf_counter()
plan = solver.interpolation_plan(G_d)
smooth = solver.interpolation_plan(G_d, mode="continuous", r=float(np.sqrt(12.0 / (np.pi * n))))
torch.cuda.synchronize()
print("two plans for %d grid points over %d models: %.1f ms, %.1f MB on the device"
      % (G_d.shape[0], n, (time.perf_counter() - t0) * 1e3, (plan.memory_used() + smooth.memory_used()) / 1e6))

no = wlsqm.number_of_dofs(2, order)
u = torch.empty(n, dtype=torch.float64, device=dev)
fk = torch.empty((n, nk), dtype=torch.float64, device=dev)
fi = torch.zeros((n, no), dtype=torch.float64, device=dev)
grid = torch.empty((3, G_d.shape[0]), dtype=torch.float64, device=dev)          # value, d/dx, d/dy on the grid
grid_smooth = torch.empty_like(grid)
want = [0, wlsqm.i2_X, wlsqm.i2_Y]


def step():
    fk.copy_(u[h_d])
    fi[:, 0] = u
    solver.solve_device(fk, fi)
    plan.evaluate(want, out=grid)                                  # the latest solve of the solver, all three diffs in one launch
    smooth.evaluate(want, out=grid_smooth)


def field(t):
    return torch.sin(np.pi * (S_d[:, 0] - t)) * torch.cos(np.pi * S_d[:, 1])


u.copy_(field(0.0))
step()                                                              # warm-up outside the capture
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
    step()
steps, dt = 100, 1e-3
torch.cuda.synchronize(); t0 = time.perf_counter()
for k in range(steps):
    u.copy_(field(k * dt))
    graph.replay()
torch.cuda.synchronize(); t_step = (time.perf_counter() - t0) / steps
t = (steps - 1) * dt
exact = torch.stack([torch.sin(np.pi * (G_d[:, 0] - t)) * torch.cos(np.pi * G_d[:, 1]),
                     np.pi * torch.cos(np.pi * (G_d[:, 0] - t)) * torch.cos(np.pi * G_d[:, 1]),
                     -np.pi * torch.sin(np.pi * (G_d[:, 0] - t)) * torch.sin(np.pi * G_d[:, 1])])
print("%d steps, one graph replay each (gather + fit + two resamplings of value and gradient): %.3f ms per step" % (steps, t_step * 1e3))
print("last step against the exact field on the grid: nearest |u| %.1e |grad| %.1e; continuous |u| %.1e |grad| %.1e"
      % (float((grid[0] - exact[0]).abs().max()), float((grid[1:] - exact[1:]).abs().max()),
         float((grid_smooth[0] - exact[0]).abs().max()), float((grid_smooth[1:] - exact[1:]).abs().max())))
eager = grid.clone()
step()
torch.cuda.synchronize()
print("eager step equals the replay bit for bit: %s" % bool(torch.equal(eager.view(torch.int64), grid.view(torch.int64))))
