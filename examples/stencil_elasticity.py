#!/usr/bin/env python3
"""A clamped plate under a body force: plane linear elasticity (Navier-Cauchy), -(mu Lap u + (lambda + mu) grad div u) = f in the unit
square and u = 0 on its boundary, on a quasi-random (Halton) cloud that comes in random order.  The two displacement components enter
each other's equations through d2/dxdy, so this is one coupled system and not two scalar solves:
wlsqm.hip.SpatialOrder puts the cloud in Morton order, knn finds the neighbours, one wlsqm.hip.StencilOperator holds the four planes
d2/dx2, d2/dxdy, d2/dy2 (zero rows on the boundary band) and `value` (the identity rows of the band, zero inside), and
wlsqm.hip.StencilSystemSolver combines them through its (2, 2, 4) coupling table and solves for both components at once (DESIGN.md
section 24).  Prints the status, the iteration count, the true residual and the largest displacement.  The size is a command-line
argument (default 20000 points); the scalar Jacobi diagonal needs more iterations as the cloud grows."""
import os, sys, time
import numpy as np
import torch
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "python-wlsqm_amd"))
import synth
import wlsqm
import wlsqm.hip

n, nk, lam, mu = (int(sys.argv[1]) if len(sys.argv) > 1 else 20000), 24, 1.0, 1.0
dev = torch.device("cuda", 0)
S_given = torch.from_numpy(np.ascontiguousarray(synth.halton(n, 2)[np.random.default_rng(0).permutation(n)])).to(dev)
order = wlsqm.hip.SpatialOrder(S_given)
S = order.take(S_given).contiguous()
h = n ** -0.5
band = torch.minimum(S, 1.0 - S).min(dim=1).values < 1.2 * h      # the clamped boundary band

hoods = wlsqm.hip.knn(S, nk)
nk_d = torch.full((n,), nk, dtype=torch.int32, device=dev)
knowns = torch.full((n,), wlsqm.b2_F, dtype=torch.int64, device=dev)
wm = torch.full((n,), wlsqm.WEIGHT_CENTER, dtype=torch.int32, device=dev)
second = wlsqm.hip.stencil_rows(2, 2, wlsqm.i2_X2, wlsqm.i2_XY, wlsqm.i2_Y2, device=dev)            # (3, 6)
rows = torch.zeros((4, n, 6), dtype=torch.float64, device=dev)
rows[:3] = torch.where(band[None, :, None], torch.zeros((), dtype=torch.float64, device=dev), second[:, None, :])
rows[3, :, wlsqm.i2_F] = band.to(torch.float64)
op = wlsqm.hip.StencilOperator(2, 2, S, hoods, nk_d, knowns, wm, rows)

# block (a, b) of M = sum_o coupling[a, b, o] A_o over the planes (X2, XY, Y2, value)
coupling = np.zeros((2, 2, 4))
coupling[0, 0] = [-(lam + 2 * mu), 0.0, -mu, 1.0]
coupling[1, 1] = [-mu, 0.0, -(lam + 2 * mu), 1.0]
coupling[0, 1] = coupling[1, 0] = [0.0, -(lam + mu), 0.0, 0.0]
solver = wlsqm.hip.StencilSystemSolver(op, coupling, diag=0.0, preconditioner="jacobi")

f = torch.zeros((n, 2), dtype=torch.float64, device=dev)         # unknowns and right-hand sides are (npoints, m), interleaved
f[:, 1] = -1.0                                                   # a uniform load in -y
f[band] = 0.0                                                    # the clamped rows: u = 0

solver.solve(f, rtol=1e-10, maxiter=4)                           # warm-up
torch.cuda.synchronize(); t0 = time.perf_counter()
info = solver.solve(f, rtol=1e-10, maxiter=20000, check_every=64)
torch.cuda.synchronize()
ms = (time.perf_counter() - t0) * 1e3
u = solver.x                                                     # the tensor that holds the solution
true = float((f - solver.product(u)[0]).norm() / f.norm())
u_given = order.restore(u)                                       # back in the caller's numbering
worst = int(u_given.norm(dim=1).argmax())
print("plane elasticity on %d points (%d clamped), lambda = %g, mu = %g" % (n, int(band.sum()), lam, mu))
print("status %d after %d iterations, %.2f ms; ||f - M u|| / ||f|| = %.2e" % (info.status, info.iterations, ms, true))
print("largest displacement %.4e at (%.3f, %.3f): u = (%.3e, %.3e)"
      % (float(u_given[worst].norm()), float(S_given[worst, 0]), float(S_given[worst, 1]), float(u_given[worst, 0]), float(u_given[worst, 1])))
print("the workspace holds %.1f MB, the operator %.1f MB" % (solver.memory_used() / 1e6, op.memory_used() / 1e6))
