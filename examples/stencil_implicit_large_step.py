#!/usr/bin/env python3
"""Backward-Euler diffusion with a LARGE step, nu dt = h^2 (tau = 1), on a quasi-random (Halton) cloud in Morton order: (I - nu dt Lap_h) u_new = u_old
with the Laplacian of the local fits as a sparse matrix (wlsqm.hip.StencilOperator) and BiCGSTAB resident on the device
(wlsqm.hip.StencilSolver).  At this step the one-sided rows near the boundary cost the matrix its positive diagonal, and the Jacobi
preconditioner needs hundreds of erratic iterations or breaks down; wlsqm.hip.BlockJacobi(16) — the exact inverses of the diagonal
blocks of 16 consecutive rows, which on a Morton-ordered cloud are 16 neighbours in space — solves it in a few dozen.  The operator
does not change during the time loop, so refresh=False factors the blocks once.  The last lines show what the feature depends on: the
same points in the order they were drawn in gain nothing."""
import os, sys, time
import numpy as np
import torch
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "python-wlsqm_amd"))
import synth
import wlsqm
import wlsqm.hip

n, nk, order, tau = 200_000, 24, 2, 1.0
dev = torch.device("cuda", 0)
S_random = synth.halton(n, 2)                                       # quasi-random: consecutive points are far apart
h2 = 1.0 / n                                                        # the square of the point spacing


def laplacian(S):
    S_d = torch.from_numpy(np.ascontiguousarray(S)).to(dev)
    hoods = wlsqm.hip.knn(S_d, nk)
    nk_d = torch.full((n,), nk, dtype=torch.int32, device=dev)
    knowns = torch.full((n,), wlsqm.b2_F, dtype=torch.int64, device=dev)
    wm = torch.full((n,), wlsqm.WEIGHT_CENTER, dtype=torch.int32, device=dev)
    return S_d, wlsqm.hip.StencilOperator(2, order, S_d, hoods, nk_d, knowns, wm, wlsqm.hip.stencil_rows(2, order, "laplacian", device=dev))


def solve_once(solver, b, maxiter=2000):
    x = torch.zeros_like(b)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    info = solver.solve(b, x, rtol=1e-10, maxiter=maxiter, check_every=16)
    torch.cuda.synchronize()
    return info, (time.perf_counter() - t0) * 1e3


S_d, lap = laplacian(S_random[synth.morton_order(S_random)])
u0 = torch.sin(np.pi * S_d[:, 0]) * torch.sin(np.pi * S_d[:, 1])
jacobi = wlsqm.hip.StencilSolver(lap, diag=1.0, scale=-tau * h2)
block = wlsqm.hip.StencilSolver(lap, diag=1.0, scale=-tau * h2, preconditioner=wlsqm.hip.BlockJacobi(16, refresh=False))
print("I - h^2 Lap_h on %d points in Morton order; the solvers hold %.1f MB (Jacobi) and %.1f MB (blocks of 16)"
      % (n, jacobi.memory_used() / 1e6, block.memory_used() / 1e6))
for name, solver in (("Jacobi", jacobi), ("BlockJacobi(16)", block)):
    solve_once(solver, u0, maxiter=4)                               # warm-up
    info, ms = solve_once(solver, u0)
    print("  %-16s status %d after %4d iterations, residual %.2e, %.2f ms" % (name, info.status, info.iterations, info.residual, ms))

# the time loop: the blocks were factored at the first start and stay; u is the initial guess and receives the solution
steps = 20
u, rhs = u0.clone(), torch.empty_like(u0)
iterations = []
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(steps):
    rhs.copy_(u)
    info = block.solve(rhs, u, rtol=1e-10, maxiter=500)
    assert info.status == 0, info
    iterations.append(info.iterations)
torch.cuda.synchronize()
exact = u0 * float(np.exp(-2.0 * np.pi ** 2 * steps * tau * h2))
inner = ((S_d - 0.5).abs() < 0.4).all(dim=1)
print("%d steps of nu dt = h^2 with BlockJacobi(16, refresh=False): %d .. %d iterations per step, %.2f ms per step; max error against "
      "the exact decay in the interior %.2e" % (steps, min(iterations), max(iterations), (time.perf_counter() - t0) / steps * 1e3,
                                                float((u - exact)[inner].abs().max())))

# the same points as they were drawn: a block of 16 consecutive rows holds no neighbours, and the preconditioner is Jacobi at a higher price
S_r, lap_r = laplacian(S_random)
b_r = torch.sin(np.pi * S_r[:, 0]) * torch.sin(np.pi * S_r[:, 1])
unordered = wlsqm.hip.StencilSolver(lap_r, diag=1.0, scale=-tau * h2, preconditioner=wlsqm.hip.BlockJacobi(16))
info, ms = solve_once(unordered, b_r)
print("the same cloud in random order, BlockJacobi(16): status %d after %d iterations, %.2f ms — order the cloud first (synth.morton_order)"
      % (info.status, info.iterations, ms))
