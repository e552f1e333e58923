#!/usr/bin/env python3
"""Two species diffusing with one backward-Euler step on a jittered cloud: (I - nu dt Lap_h) u_new = u_old for both at once.  The matrix is
the same for the two, so a solver made with nfields=2 (wlsqm.hip.StencilSolver.solve_many) solves them as two independent BiCGSTAB
recurrences that share every pass over the matrix: each species stops at its own iteration count and is left alone from then on, and its
bits are those of a single-field solve of that species.  Also the gradient of a loss on both species with respect to the old state
(wlsqm.hip.differentiable_stencil_solve_many): one stacked transposed solve."""
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
# a jittered cloud in Morton order would serve a BlockJacobi; the default Jacobi preconditioner does not mind the order
ij = np.stack(np.meshgrid(np.arange(m), np.arange(m), indexing="ij"), axis=-1).reshape(n, 2)
S_d = torch.from_numpy((ij + 0.5 + 0.5 * (rng.random((n, 2)) - 0.5)) / m).to(dev)
hoods = wlsqm.hip.knn(S_d, nk)
nk_d = torch.full((n,), nk, dtype=torch.int32, device=dev)
knowns = torch.full((n,), wlsqm.b2_F, dtype=torch.int64, device=dev)
wm = torch.full((n,), wlsqm.WEIGHT_CENTER, dtype=torch.int32, device=dev)
h2 = 1.0 / n
band = (torch.minimum(S_d, 1.0 - S_d).min(dim=1).values < 1.5 * h2 ** 0.5)
rows = wlsqm.hip.stencil_rows(2, order, "laplacian", device=dev).expand(n, -1).clone()
rows[band] = 0.0                                                    # Dirichlet rows: the identity in M
lap = wlsqm.hip.StencilOperator(2, order, S_d, hoods, nk_d, knowns, wm, rows[None])
nu_dt = 0.25 * h2
both = wlsqm.hip.StencilSolver(lap, diag=1.0, scale=-nu_dt, nfields=2)
one = wlsqm.hip.StencilSolver(lap, diag=1.0, scale=-nu_dt)
print("two species on %d points: workspace %.1f MB for the stacked solver, %.1f MB for a single-field one"
      % (n, both.memory_used() / 1e6, one.memory_used() / 1e6))

# species 0 is smooth, species 1 has a sharp front: they need different numbers of iterations
x, y = S_d[:, 0], S_d[:, 1]
old = torch.stack([torch.sin(np.pi * x) * torch.sin(np.pi * y), torch.tanh(40.0 * (x - 0.5)) * torch.sin(np.pi * y)])
new = old.clone()                                                   # the initial guess, and the solution
infos = both.solve_many(old, new, rtol=1e-10, maxiter=200)
assert all(info.status == 0 for info in infos), infos
alone = old.clone()
alone_infos = [one.solve(old[f], alone[f], rtol=1e-10, maxiter=200) for f in range(2)]
print("one step: species 0 in %d iterations, species 1 in %d; the same bits as two single solves: %s"
      % (infos[0].iterations, infos[1].iterations, bool(torch.equal(new, alone)) and infos == alone_infos))


def timed(fn, reps=20):
    fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


iters = max(info.iterations for info in infos)
t_both = timed(lambda: (new.copy_(old), both.enqueue_many(old, new, iters)))
t_alone = timed(lambda: (alone.copy_(old), [one.enqueue(old[f], alone[f], iters) for f in range(2)]))
print("enqueued, %d iterations: stacked %.3f ms per step, two single solves %.3f ms" % (iters, t_both, t_alone))

# dL/d(old) of a loss on both species, through the step
target = 0.9 * old
b = old.clone().requires_grad_(True)
u = wlsqm.hip.differentiable_stencil_solve_many(both, b, rtol=1e-10, maxiter=200)
loss = 0.5 * ((u - target) ** 2).sum()
loss.backward()
adjoint = both.info_many()
print("loss %.6e; dL/d(old) by one stacked transposed solve (%d and %d iterations), |grad| = %.3e"
      % (float(loss.detach()), adjoint[0].iterations, adjoint[1].iterations, float(b.grad.norm())))
