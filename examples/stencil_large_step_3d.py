#!/usr/bin/env python3
"""Backward-Euler diffusion in 3D with a LARGE step, nu dt = h^2 (tau = 1), on a quasi-random (Halton) cloud in Morton order:
(I - nu dt Lap_h) u_new = u_old with the Laplacian of the local fits as a sparse matrix (wlsqm.hip.StencilOperator).  In 3D the
one-sided rows near the boundary make this matrix indefinite enough that BiCGSTAB breaks down or wanders, with the Jacobi diagonal and
with wlsqm.hip.BlockJacobi(16) alike.  method="bicgstab2" — two BiCG steps, then one residual minimisation over a two-dimensional
space — converges on the same matrix with the same blocks, in the same kernels' passes: nothing else changes in
the calling code.  `iterations` counts pairs of matrix products for both methods, so the two counts below compare directly.
This is ONE step: the example is about solving the system.  (An indefinite step matrix also says something about the scheme: at this
step size the boundary rows of the cloud amplify some modes, and a time loop on it would want a smaller step or boundary conditions.)
The size is a command-line argument (default 2000 points); the iteration count grows quickly with it, DESIGN.md section 21 says how far
the method reaches."""
import os, sys, time
import numpy as np
import torch
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "python-wlsqm_amd"))
import synth
import wlsqm
import wlsqm.hip

n, nk, order, tau = (int(sys.argv[1]) if len(sys.argv) > 1 else 2000), 40, 2, 1.0
dev = torch.device("cuda", 0)
S = synth.halton(n, 3)
S_d = torch.from_numpy(np.ascontiguousarray(S[synth.morton_order(S)])).to(dev)      # consecutive rows are neighbours in space
h2 = n ** (-2.0 / 3.0)                                              # the square of the point spacing

hoods = wlsqm.hip.knn(S_d, nk)
nk_d = torch.full((n,), nk, dtype=torch.int32, device=dev)
knowns = torch.full((n,), wlsqm.b3_F, dtype=torch.int64, device=dev)
wm = torch.full((n,), wlsqm.WEIGHT_CENTER, dtype=torch.int32, device=dev)
lap = wlsqm.hip.StencilOperator(3, order, S_d, hoods, nk_d, knowns, wm, wlsqm.hip.stencil_rows(3, order, "laplacian", device=dev))


def solve_once(solver, b, maxiter=6000):
    x = torch.zeros_like(b)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    info = solver.solve(b, x, rtol=1e-10, maxiter=maxiter, check_every=64)
    torch.cuda.synchronize()
    return x, info, (time.perf_counter() - t0) * 1e3


u0 = torch.sin(np.pi * S_d[:, 0]) * torch.sin(np.pi * S_d[:, 1]) * torch.sin(np.pi * S_d[:, 2])
solvers = {method: wlsqm.hip.StencilSolver(lap, diag=1.0, scale=-tau * h2, preconditioner=wlsqm.hip.BlockJacobi(16, refresh=False), method=method)
           for method in ("bicgstab", "bicgstab2")}
print("I - h^2 Lap_h on %d points of the unit cube in Morton order, blocks of 16" % n)
for method, solver in solvers.items():
    solve_once(solver, u0, maxiter=4)                               # warm-up
    x, info, ms = solve_once(solver, u0)
    true = float((u0 - solver.product(x)[0]).norm() / u0.norm())
    print("  %-10s status %d after %4d iterations, ||b - M x|| / ||b|| = %.2e, %.2f ms" % (method, info.status, info.iterations, true, ms))
print("one step: max |u_new - u_old| = %.3e" % float((x - u0).abs().max()))
