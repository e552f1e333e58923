#!/usr/bin/env python3
"""Backward-Euler diffusion u_t = nu Lap u on a jittered cloud, the boundary values held: every step solves (I - nu dt Lap_h) u_new = u_old
with the Laplacian of the local fits as a sparse matrix (wlsqm.hip.StencilOperator) and BiCGSTAB resident on the device (wlsqm.hip.StencilSolver: eight launches
per iteration, every dot product formed in the pass that makes its vector, the stop taken on the device).  Runs eager — solve() reads the
iteration count every 8 iterations — and as one HIP graph replay per step: enqueue() is kernel launches only, a fixed number of
iterations of which the ones behind the stop return at once.  Both give the same bits."""
import os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "python-wlsqm_amd"))
import wlsqm
import wlsqm.hip

m, nk, order = 448, 24, 2
n = m * m
rng = np.random.default_rng(1)
dev = torch.device("cuda", 0)
# a jittered cloud: one point in every cell of an m x m grid, anywhere in the cell's middle half.  (Uniformly random points leave a few
# lopsided neighbourhoods whose Laplacian has the wrong sign on the diagonal; backward Euler amplifies those.)
ij = np.stack(np.meshgrid(np.arange(m), np.arange(m), indexing="ij"), axis=-1).reshape(n, 2)
S_d = torch.from_numpy((ij + 0.5 + 0.5 * (rng.random((n, 2)) - 0.5)) / m).to(dev)
hoods = wlsqm.hip.knn(S_d, nk)
nk_d = torch.full((n,), nk, dtype=torch.int32, device=dev)
knowns = torch.full((n,), wlsqm.b2_F, dtype=torch.int64, device=dev)
wm = torch.full((n,), wlsqm.WEIGHT_CENTER, dtype=torch.int32, device=dev)

# Dirichlet rows: within 1.5 spacings of the boundary the neighbourhoods are one-sided; those rows get the zero operator, so that M's
# row is the identity and u stays as it is
h2 = 1.0 / n                                                        # the square of the point spacing
band = (torch.minimum(S_d, 1.0 - S_d).min(dim=1).values < 1.5 * h2 ** 0.5)
rows = wlsqm.hip.stencil_rows(2, order, "laplacian", device=dev).expand(n, -1).clone()
rows[band] = 0.0
lap = wlsqm.hip.StencilOperator(2, order, S_d, hoods, nk_d, knowns, wm, rows[None])
nu_dt = 0.25 * h2
solver = wlsqm.hip.StencilSolver(lap, diag=1.0, scale=-nu_dt)       # M = I - nu dt Lap_h, Jacobi-preconditioned
print("Laplacian on %d points (%d of them Dirichlet rows): %.1f MB, fill %.3f; solver workspace %.1f MB" % (n, int(band.sum()), lap.memory_used() / 1e6, lap.fill, solver.memory_used() / 1e6))

u0 = torch.sin(np.pi * S_d[:, 0]) * torch.sin(np.pi * S_d[:, 1])
steps, rtol = 50, 1e-10
u, rhs = u0.clone(), torch.empty_like(u0)

# eager: u is the initial guess and receives the solution
iterations = []
u.copy_(u0)
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(steps):
    rhs.copy_(u)
    info = solver.solve(rhs, u, rtol=rtol, maxiter=200)
    assert info.status == 0, info
    iterations.append(info.iterations)
torch.cuda.synchronize(); t_eager = (time.perf_counter() - t0) / steps
u_eager = u.clone()
enqueued = max(iterations) + 4                                      # what the graph enqueues per step: a few more than any step needed


def step():
    rhs.copy_(u)
    solver.enqueue(rhs, u, enqueued, rtol=rtol)


u.copy_(u0)
step()                                                              # warm-up outside the capture
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
    step()
u.copy_(u0)
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(steps):
    graph.replay()
torch.cuda.synchronize(); t_graph = (time.perf_counter() - t0) / steps
last = solver.info()

inner = ((S_d - 0.5).abs() < 0.4).all(dim=1)
exact = u0 * float(np.exp(-2.0 * np.pi ** 2 * steps * nu_dt))
print("backward Euler, %d steps of nu dt = h^2 / 4: %d .. %d iterations per step to rtol %.0e; eager solve %.3f ms per step, one HIP graph "
      "replay of %d enqueued iterations %.3f ms (identical: %s; last step: status %d after %d iterations)"
      % (steps, min(iterations), max(iterations), rtol, t_eager * 1e3, enqueued, t_graph * 1e3, bool(torch.equal(u, u_eager)), last.status,
         last.iterations))
print("max error against the exact decay in the interior %.2e (the field decayed by %.2e)"
      % (float((u - exact)[inner].abs().max()), float((u0 - exact)[inner].abs().max())))
