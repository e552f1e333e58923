#!/usr/bin/env python3
"""The clamped plate of stencil_elasticity.py — plane linear elasticity, -(mu Lap u + (lambda + mu) grad div u) = f in the unit square,
u = 0 on its boundary, on a Halton cloud put in Morton order — solved twice on one operator: with the scalar Jacobi diagonal of
wlsqm.hip.StencilSystemSolver and with wlsqm.hip.PointBlockJacobi(points), the exact inverses of the diagonal blocks of `points`
consecutive points with both displacement components of each.  On a cloud in Morton order consecutive points
are neighbours, so a block holds a patch of the plate and its couplings; the gain grows with the cloud.  Prints, per preconditioner,
the status, the iteration count, the time and the true residual.  Arguments: the number of points (default 20000) and the points of a
block (default 8; 2 points <= 32)."""
import os, sys, time
import numpy as np
import torch
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "python-wlsqm_amd"))
import synth
import wlsqm
import wlsqm.hip

n = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
points = int(sys.argv[2]) if len(sys.argv) > 2 else 8
nk, lam, mu = 24, 1.0, 1.0
dev = torch.device("cuda", 0)
S_given = torch.from_numpy(np.ascontiguousarray(synth.halton(n, 2)[np.random.default_rng(0).permutation(n)])).to(dev)
order = wlsqm.hip.SpatialOrder(S_given)
S = order.take(S_given).contiguous()
band = torch.minimum(S, 1.0 - S).min(dim=1).values < 1.2 * n ** -0.5      # the clamped boundary band

hoods = wlsqm.hip.knn(S, nk)
nk_d = torch.full((n,), nk, dtype=torch.int32, device=dev)
knowns = torch.full((n,), wlsqm.b2_F, dtype=torch.int64, device=dev)
wm = torch.full((n,), wlsqm.WEIGHT_CENTER, dtype=torch.int32, device=dev)
second = wlsqm.hip.stencil_rows(2, 2, wlsqm.i2_X2, wlsqm.i2_XY, wlsqm.i2_Y2, device=dev)
rows = torch.zeros((4, n, 6), dtype=torch.float64, device=dev)
rows[:3] = torch.where(band[None, :, None], torch.zeros((), dtype=torch.float64, device=dev), second[:, None, :])
rows[3, :, wlsqm.i2_F] = band.to(torch.float64)
op = wlsqm.hip.StencilOperator(2, 2, S, hoods, nk_d, knowns, wm, rows)

coupling = np.zeros((2, 2, 4))                                   # the planes (X2, XY, Y2, value)
coupling[0, 0] = [-(lam + 2 * mu), 0.0, -mu, 1.0]
coupling[1, 1] = [-mu, 0.0, -(lam + 2 * mu), 1.0]
coupling[0, 1] = coupling[1, 0] = [0.0, -(lam + mu), 0.0, 0.0]

f = torch.zeros((n, 2), dtype=torch.float64, device=dev)
f[:, 1] = -1.0                                                   # a uniform load in -y
f[band] = 0.0                                                    # the clamped rows: u = 0

print("plane elasticity on %d points in Morton order (%d clamped), lambda = %g, mu = %g" % (n, int(band.sum()), lam, mu))
for name, pc in (("jacobi", "jacobi"), ("blocks of %d points" % points, wlsqm.hip.PointBlockJacobi(points))):
    solver = wlsqm.hip.StencilSystemSolver(op, coupling, diag=0.0, preconditioner=pc)
    solver.solve(f, rtol=1e-10, maxiter=4)                       # warm-up
    torch.cuda.synchronize(); t0 = time.perf_counter()
    info = solver.solve(f, rtol=1e-10, maxiter=20000, check_every=64)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    true = float((f - solver.product(solver.x)[0]).norm() / f.norm())
    print("%-20s status %d after %5d iterations, %8.2f ms; ||f - M u|| / ||f|| = %.2e; the solver holds %.1f MB"
          % (name, info.status, info.iterations, ms, true, solver.memory_used() / 1e6))
    solver.close()
