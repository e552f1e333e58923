#!/usr/bin/env python3
"""The advection loop of time_stepping_device.py with the differential operator as a sparse matrix: d/dx of the local fits is built
once (wlsqm.hip.StencilOperator), and a forward-Euler step u <- u - dt u_x is then ONE kernel, apply(..., out=u, alpha=-dt, beta=1.0),
instead of a gather, a solve for all DOFs and an update.  Runs eager and as one HIP graph replay per step, and prints its agreement
with the solver route."""
import os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "python-wlsqm_amd"))
import wlsqm
import wlsqm.hip

n, nk, order = 200_000, 32, 2
rng = np.random.default_rng(1)
dev = torch.device("cuda", 0)
S_d = torch.from_numpy(rng.uniform(0.0, 1.0, (n, 2))).to(dev)
hoods = wlsqm.hip.knn(S_d, nk)                                      # nk nearest neighbours of every point, on the GPU
nk_d = torch.full((n,), nk, dtype=torch.int32, device=dev)
knowns = torch.full((n,), wlsqm.b2_F, dtype=torch.int64, device=dev)
wm = torch.full((n,), wlsqm.WEIGHT_CENTER, dtype=torch.int32, device=dev)

# the operator: one row per point, its neighbours' coefficients and (the function value is a known of the fit) the point's own
t0 = time.perf_counter()
ddx = wlsqm.hip.StencilOperator(2, order, S_d, hoods, nk_d, knowns, wm, wlsqm.hip.stencil_rows(2, order, wlsqm.i2_X, device=dev))
torch.cuda.synchronize()
print("d/dx on %d points: built in %.1f ms, %.1f MB, fill %.3f" % (n, (time.perf_counter() - t0) * 1e3, ddx.memory_used() / 1e6, ddx.fill))

u0 = torch.sin(np.pi * S_d[:, 0]) * torch.cos(np.pi * S_d[:, 1])
steps, dt = 200, 2e-5
u, v = u0.clone(), torch.empty_like(u0)


def advect():
    v.copy_(u)                                                      # the product does not run in place: out must not overlap its input
    ddx.apply(v, out=u.view(1, n), alpha=-dt, beta=1.0)


advect()                                                            # warm-up outside the capture
u.copy_(u0)
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(steps):
    advect()
torch.cuda.synchronize(); t_eager = (time.perf_counter() - t0) / steps
u_eager = u.clone()
u.copy_(u0)
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
    advect()
u.copy_(u0)
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(steps):
    graph.replay()
torch.cuda.synchronize(); t_graph = (time.perf_counter() - t0) / steps
u_stencil = u.clone()

# the solver route of time_stepping_device.py: gather, solve for every DOF, use one column
h64 = hoods.long()
solver = wlsqm.ExpertSolver(dimension=2, nk=np.full(n, nk, np.int32), order=np.full(n, order, np.int32),
                            knowns=np.full(n, wlsqm.b2_F, np.int64), weighting_method=np.full(n, wlsqm.WEIGHT_CENTER, np.int32))
solver.prepare_device(S_d, S_d[h64].contiguous())
fi = torch.zeros((n, wlsqm.number_of_dofs(2, order)), dtype=torch.float64, device=dev)
fk_buf = torch.empty((n, nk), dtype=torch.float64, device=dev)
u.copy_(u0)
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(steps):
    fk_buf.copy_(u[h64])
    fi[:, 0] = u
    solver.solve_device(fk_buf, fi)
    u.sub_(dt * fi[:, wlsqm.i2_X])
torch.cuda.synchronize(); t_solver = (time.perf_counter() - t0) / steps

inner = ((S_d - 0.5).abs() < 0.45).all(dim=1)
exact = torch.sin(np.pi * (S_d[:, 0] - steps * dt)) * torch.cos(np.pi * S_d[:, 1])
print("forward-Euler advection, %d steps: stencil eager %.3f ms per step, one HIP graph replay per step %.3f ms (identical: %s), "
      "gather + solve + update %.3f ms" % (steps, t_eager * 1e3, t_graph * 1e3, bool(torch.equal(u_stencil, u_eager)), t_solver * 1e3))
print("stencil against the solver route: max |difference| %.2e; max error against the exact solution %.2e (solver route: %.2e)"
      % (float((u_stencil - u).abs().max()), float((u_stencil - exact)[inner].abs().max()), float((u - exact)[inner].abs().max())))
