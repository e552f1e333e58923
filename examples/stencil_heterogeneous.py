#!/usr/bin/env python3
"""A material that varies in space: plane linear elasticity on a clamped plate (examples/stencil_elasticity.py) with a stiff
circular inclusion, stated by a per-point coupling tensor (2, 2, 4, npoints).
  1. The elastic inclusion.  mu(x) and lambda(x) are 4 times the matrix's inside a disc of radius 0.2 (smoothed over two point
     spacings); the equation of point i carries its own Lame parameters, -(mu Lap u + (lambda + mu) grad div u) = f (the terms with
     the gradients of the parameters are left out: this is the pointwise-homogeneous model).  The plate sags less under the inclusion.
  2. A stiffness field recovered by gradient descent.  The displacement observed for the inclusion is matched from a homogeneous
     start by Adam on a per-point log-stiffness s(x): mu = exp(s), lambda = exp(s).  The tensor is a torch expression of s, and
     wlsqm.hip.differentiable_stencil_system_solve carries the loss through the solve to all of its 16 npoints entries: one transposed
     solve, one stacked product and one elementwise product per backward pass.
The size is a command-line argument (default 2000 points)."""
import os, sys
import numpy as np
import torch
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "python-wlsqm_amd"))
import synth
import wlsqm
import wlsqm.hip

n, nk = (int(sys.argv[1]) if len(sys.argv) > 1 else 2000), 24
dev = torch.device("cuda", 0)
f64 = dict(dtype=torch.float64, device=dev)
S0 = torch.from_numpy(np.ascontiguousarray(synth.halton(n, 2))).to(dev)
S = wlsqm.hip.SpatialOrder(S0).take(S0).contiguous()
h = n ** -0.5
band = torch.minimum(S, 1.0 - S).min(dim=1).values < 1.2 * h             # the clamped boundary band

hoods = wlsqm.hip.knn(S, nk)
nk_d = torch.full((n,), nk, dtype=torch.int32, device=dev)
knowns = torch.full((n,), wlsqm.b2_F, dtype=torch.int64, device=dev)
wm = torch.full((n,), wlsqm.WEIGHT_CENTER, dtype=torch.int32, device=dev)
second = wlsqm.hip.stencil_rows(2, 2, wlsqm.i2_X2, wlsqm.i2_XY, wlsqm.i2_Y2, device=dev)
rows = torch.zeros((4, n, 6), **f64)
rows[:3] = torch.where(band[None, :, None], torch.zeros((), **f64), second[:, None, :])
rows[3, :, wlsqm.i2_F] = band.to(torch.float64)
op = wlsqm.hip.StencilOperator(2, 2, S, hoods, nk_d, knowns, wm, rows)


def table(lam, mu):
    """The coupling tensor (2, 2, 4, n) over the planes (X2, XY, Y2, value) as a differentiable function of the fields lam, mu (n,)."""
    zero, one = torch.zeros_like(mu), torch.ones_like(mu)
    return torch.stack([torch.stack([torch.stack([-(lam + 2 * mu), zero, -mu, one]), torch.stack([zero, -(lam + mu), zero, zero])]),
                        torch.stack([torch.stack([zero, -(lam + mu), zero, zero]), torch.stack([-mu, zero, -(lam + 2 * mu), one])])]).contiguous()


f = torch.zeros((n, 2), **f64)
f[:, 1] = -1.0
f[band] = 0.0
r = ((S - 0.5) ** 2).sum(dim=1).sqrt()
inclusion = 1.0 + 3.0 * torch.sigmoid((0.2 - r) / (2.0 * h))              # 4 inside the disc, 1 outside
ones = torch.ones((n,), **f64)
solver = wlsqm.hip.StencilSystemSolver(op, table(ones, ones))
solve = lambda cp: wlsqm.hip.differentiable_stencil_system_solve(solver, f, coupling=cp, rtol=1e-10, maxiter=20000, check_every=32)

# 1. the plate with and without the inclusion
with torch.no_grad():
    plain = solve(table(ones, ones)).clone()
    observed = solve(table(inclusion, inclusion)).clone()
centre = int(r.argmin())
print("plane elasticity on %d points (%d clamped), inclusion of radius 0.2 and 4 times the stiffness" % (n, int(band.sum())))
print("vertical displacement at the centre: homogeneous %.5e, with the inclusion %.5e (%d iterations)"
      % (float(plain[centre, 1]), float(observed[centre, 1]), solver.info().iterations))

# 2. recover the stiffness field from the observed displacement
s = torch.zeros((n,), **f64).requires_grad_()                             # log-stiffness, a homogeneous start
opt = torch.optim.Adam([s], lr=0.05)
inside, outside = r < 0.12, r > 0.3
for it in range(301):
    opt.zero_grad()
    u = solve(table(torch.exp(s), torch.exp(s)))
    forward = solver.info().iterations
    loss = ((u - observed) ** 2).sum() / (observed ** 2).sum()
    loss.backward()
    if it % 50 == 0:
        k = torch.exp(s.detach())
        print("step %3d: relative misfit %.3e, mean stiffness inside %.3f (true %.3f), outside %.3f (true %.3f) (forward %d, adjoint %d iterations)"
              % (it, float(loss.detach()), float(k[inside].mean()), float(inclusion[inside].mean()), float(k[outside & ~band].mean()),
                 float(inclusion[outside & ~band].mean()), forward, solver.info().iterations))
    opt.step()
