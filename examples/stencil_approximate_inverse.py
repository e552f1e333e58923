#!/usr/bin/env python3
"""The 3D step that the other preconditioners cannot do: backward-Euler diffusion with nu dt = h^2 (tau = 1) on a quasi-random (Halton)
cloud of the unit cube in Morton order, (I - nu dt Lap_h) u_new = u_old with the Laplacian of the local fits as a sparse matrix
(wlsqm.hip.StencilOperator).  With the Jacobi diagonal BiCGSTAB does not get there at all, with wlsqm.hip.BlockJacobi(16) it breaks down
or takes a thousand iterations (examples/stencil_large_step_3d.py), and both grow quickly with the size of the cloud.
wlsqm.hip.ApproximateInverse() preconditions with a sparse approximate inverse Q on the matrix's own pattern — row i of Q minimises
||q^T M - e_i^T||, one small dense least-squares problem per point, solved on the device — which couples every
point with all its neighbours: a few dozen iterations with either method.  An iteration costs about twice a Jacobi iteration, and the
build of Q costs hundreds of them: refresh=False builds it once for a time loop on a fixed operator (solver.refresh() after the cloud
moves).  The size is a command-line argument (default 20000 points)."""
import os, sys, time
import numpy as np
import torch
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "python-wlsqm_amd"))
import synth
import wlsqm
import wlsqm.hip

n, nk, order, tau = (int(sys.argv[1]) if len(sys.argv) > 1 else 20000), 40, 2, 1.0
dev = torch.device("cuda", 0)
S = synth.halton(n, 3)
S_d = torch.from_numpy(np.ascontiguousarray(S[synth.morton_order(S)])).to(dev)
h2 = n ** (-2.0 / 3.0)                                              # the square of the point spacing

hoods = wlsqm.hip.knn(S_d, nk)
nk_d = torch.full((n,), nk, dtype=torch.int32, device=dev)
knowns = torch.full((n,), wlsqm.b3_F, dtype=torch.int64, device=dev)
wm = torch.full((n,), wlsqm.WEIGHT_CENTER, dtype=torch.int32, device=dev)
lap = wlsqm.hip.StencilOperator(3, order, S_d, hoods, nk_d, knowns, wm, wlsqm.hip.stencil_rows(3, order, "laplacian", device=dev))


def solve_once(solver, b, maxiter=3000):
    x = torch.zeros_like(b)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    info = solver.solve(b, x, rtol=1e-10, maxiter=maxiter, check_every=64)
    torch.cuda.synchronize()
    return x, info, (time.perf_counter() - t0) * 1e3


u0 = torch.sin(np.pi * S_d[:, 0]) * torch.sin(np.pi * S_d[:, 1]) * torch.sin(np.pi * S_d[:, 2])
routes = [("BlockJacobi(16)", wlsqm.hip.BlockJacobi(16, refresh=False), "bicgstab2"),
          ("ApproximateInverse", wlsqm.hip.ApproximateInverse(refresh=False), "bicgstab2"),
          ("ApproximateInverse", wlsqm.hip.ApproximateInverse(refresh=False), "bicgstab")]
print("I - h^2 Lap_h on %d points of the unit cube in Morton order" % n)
for name, preconditioner, method in routes:
    solver = wlsqm.hip.StencilSolver(lap, diag=1.0, scale=-tau * h2, preconditioner=preconditioner, method=method)
    solve_once(solver, u0, maxiter=4)                               # warm-up; builds the preconditioner once
    x, info, ms = solve_once(solver, u0)
    true = float((u0 - solver.product(x)[0]).norm() / u0.norm())
    print("  %-18s %-9s status %d after %4d iterations, ||b - M x|| / ||b|| = %.2e, %.2f ms"
          % (name, method, info.status, info.iterations, true, ms))
    if name == "ApproximateInverse" and method == "bicgstab":
        Q = solver.preconditioner_matrix()
        r = torch.randn(n, dtype=torch.float64, device=dev)
        print("  Q has %d entries; ||Q M r - r|| / ||r|| = %.2f for a random r (an exact inverse would give 0)"
              % (Q.values().numel(), float((solver.precondition(solver.product(r)[0]) - r).norm() / r.norm())))
    solver.close()
print("one step: max |u_new - u_old| = %.3e" % float((x - u0).abs().max()))
