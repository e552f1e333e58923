#!/usr/bin/env python3
"""Gradients through a coupled solve: plane linear elasticity on a clamped plate (examples/stencil_elasticity.py), differentiated.
  1. Material identification.  The Lame constants enter M only through the (2, 2, 4) coupling table; a displacement field observed for
     lambda = 1.6, mu = 0.7 is matched by gradient descent (Adam) on (lambda, mu) from a wrong start.  The table is a torch expression
     of the two constants, and wlsqm.hip.differentiable_stencil_system_solve carries the loss through the solve to it: one transposed
     solve and one stacked product per backward pass.
  2. Shape sensitivity.  dL/dS of the compliance L = f . u at fixed neighbour lists: how the work of the load changes when a node
     moves.  Printed for the node where it is largest.
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
S0 = torch.from_numpy(np.ascontiguousarray(synth.halton(n, 2))).to(dev)
S = wlsqm.hip.SpatialOrder(S0).take(S0).contiguous()
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


def table(lam, mu):
    """The coupling table (2, 2, 4) over the planes (X2, XY, Y2, value) as a differentiable function of the Lame constants."""
    zero, one = torch.zeros((), dtype=torch.float64), torch.ones((), dtype=torch.float64)
    return torch.stack([torch.stack([torch.stack([-(lam + 2 * mu), zero, -mu, one]), torch.stack([zero, -(lam + mu), zero, zero])]),
                        torch.stack([torch.stack([zero, -(lam + mu), zero, zero]), torch.stack([-mu, zero, -(lam + 2 * mu), one])])])


f = torch.zeros((n, 2), dtype=torch.float64, device=dev)
f[:, 1] = -1.0
f[band] = 0.0
solver = wlsqm.hip.StencilSystemSolver(op, table(torch.tensor(1.0, dtype=torch.float64), torch.tensor(1.0, dtype=torch.float64)).numpy())
solve = lambda cp, **kw: wlsqm.hip.differentiable_stencil_system_solve(solver, f, coupling=cp, rtol=1e-10, maxiter=20000, check_every=32, **kw)

# 1. recover (lambda, mu) from an observed displacement field
with torch.no_grad():
    observed = solve(table(torch.tensor(1.6, dtype=torch.float64), torch.tensor(0.7, dtype=torch.float64))).clone()
theta = torch.tensor([1.0, 1.0], dtype=torch.float64, requires_grad=True)      # (lambda, mu), a wrong start
opt = torch.optim.Adam([theta], lr=0.05)
print("plane elasticity on %d points (%d clamped); observed with lambda = 1.6, mu = 0.7" % (n, int(band.sum())))
for it in range(401):
    opt.zero_grad()
    u = solve(table(theta[0], theta[1]))
    forward = solver.info().iterations
    loss = ((u - observed) ** 2).sum() / (observed ** 2).sum()
    loss.backward()
    if it % 50 == 0:
        print("step %3d: lambda = %.4f, mu = %.4f, relative misfit %.3e (forward %d, adjoint %d iterations)"
              % (it, float(theta.detach()[0]), float(theta.detach()[1]), float(loss.detach()), forward, solver.info().iterations))
    opt.step()

# 2. the sensitivity of the compliance to the node positions, at the recovered constants
Sg = S.clone().requires_grad_()
u = solve(table(theta[0].detach(), theta[1].detach()), S=Sg)
compliance = (f * u).sum()
compliance.backward()
g = Sg.grad
worst = int(g.norm(dim=1).argmax())
print("compliance f . u = %.6e; |d compliance / dS| is largest at node (%.3f, %.3f): (%.3e, %.3e)"
      % (float(compliance.detach()), float(S[worst, 0]), float(S[worst, 1]), float(g[worst, 0]), float(g[worst, 1])))
