#!/usr/bin/env python3
"""An inverse problem on an implicit scheme: recover the reaction field r(x) of one backward-Euler step of u_t = nu Lap u - r u,
(diag(1 + dt r) - nu dt Lap_h) u_new = u_old, from observations of u_new — and then fit three node positions to the same kind of data
(the misfit falls by four orders; one step's data determine a position only weakly, as the distance printed at the end shows).
wlsqm.hip.differentiable_stencil_solve puts StencilSolver.solve into an autograd graph: the backward pass solves the transposed
system once (solve(transpose=True)) and the gradients with respect to the diag tensor, the right-hand side and the point table come from
it.  torch.optim does the rest."""
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "python-wlsqm_amd"))
import wlsqm
import wlsqm.hip

m, nk, order = 24, 24, 2
n = m * m
rng = np.random.default_rng(3)
dev = torch.device("cuda", 0)
# a jittered cloud, as examples/stencil_implicit_diffusion.py; Dirichlet rows (the zero operator) in a band along the boundary
ij = np.stack(np.meshgrid(np.arange(m), np.arange(m), indexing="ij"), axis=-1).reshape(n, 2)
S = torch.from_numpy((ij + 0.5 + 0.5 * (rng.random((n, 2)) - 0.5)) / m).to(dev)
hoods = wlsqm.hip.knn(S, nk)
nk_d = torch.full((n,), nk, dtype=torch.int32, device=dev)
knowns = torch.full((n,), wlsqm.b2_F, dtype=torch.int64, device=dev)
wm = torch.full((n,), wlsqm.WEIGHT_CENTER, dtype=torch.int32, device=dev)
h2 = 1.0 / n
band = torch.minimum(S, 1.0 - S).min(dim=1).values < 1.5 * h2 ** 0.5
rows = wlsqm.hip.stencil_rows(2, order, "laplacian", device=dev).expand(n, -1).clone()
rows[band] = 0.0
lap = wlsqm.hip.StencilOperator(2, order, S, hoods, nk_d, knowns, wm, rows[None])
lap.prepare_transpose()
nu_dt, dt = 4.0 * h2, 0.5
u_old = torch.sin(np.pi * S[:, 0]) * torch.sin(np.pi * S[:, 1]) + 0.5

# ---- 1. the reaction field ----
r_true = 1.0 + torch.exp(-((S[:, 0] - 0.35) ** 2 + (S[:, 1] - 0.6) ** 2) / 0.03)
truth = wlsqm.hip.StencilSolver(lap, diag=1.0 + dt * r_true, scale=-nu_dt)
observed = torch.zeros(n, dtype=torch.float64, device=dev)
assert truth.solve(u_old, observed, rtol=1e-12).status == 0

r = torch.ones(n, dtype=torch.float64, device=dev, requires_grad=True)
diag = torch.empty(n, dtype=torch.float64, device=dev, requires_grad=True)   # the solver reads this tensor at every solve; the loop refills it
solver = wlsqm.hip.StencilSolver(lap, diag=diag, scale=-nu_dt)
opt = torch.optim.LBFGS([r], max_iter=100, tolerance_grad=1e-14, tolerance_change=1e-16, line_search_fn="strong_wolfe")


def closure():
    opt.zero_grad()
    with torch.no_grad():
        diag.copy_(1.0 + dt * r)
    diag.grad = None
    u_new = wlsqm.hip.differentiable_stencil_solve(solver, u_old, rtol=1e-12)
    loss = ((u_new - observed) ** 2).sum()
    loss.backward()                                                 # dL/d(diag) by the adjoint solve ...
    r.grad = dt * diag.grad                                         # ... and the chain rule of diag = 1 + dt r by hand (diag is the leaf)
    return loss


first = float(closure().detach())
opt.step(closure)
last = float(closure().detach())
inner = ~band
err = float((r.detach() - r_true)[inner].abs().max())
print("reaction field on %d points: misfit %.3e -> %.3e, max |r - r_true| off the boundary band %.3e" % (n, first, last, err))
assert last < 1e-4 * first

# ---- 2. a few node positions ----
moved = torch.tensor([n // 2 + 3, n // 3 + 5, 2 * n // 3 + 7], device=dev)
S_true = S.clone()
S_true[moved] += 0.2 * h2 ** 0.5 * torch.tensor([[1.0, -0.5], [-0.7, 0.6], [0.4, 0.9]], dtype=torch.float64, device=dev)
plain = wlsqm.hip.StencilSolver(lap, diag=1.0 + dt, scale=-nu_dt)
lap.update(S_true)
assert plain.solve(u_old, observed, rtol=1e-12).status == 0

offset = torch.zeros((3, 2), dtype=torch.float64, device=dev, requires_grad=True)
opt = torch.optim.LBFGS([offset], max_iter=100, tolerance_grad=1e-16, tolerance_change=1e-18, line_search_fn="strong_wolfe")


def closure_S():
    opt.zero_grad()
    S_now = S.index_add(0, moved, offset)                           # autograd carries dL/dS back to the three offsets
    u_new = wlsqm.hip.differentiable_stencil_solve(plain, u_old, S=S_now.contiguous(), rtol=1e-12)
    loss = ((u_new - observed) ** 2).sum()
    loss.backward()
    return loss


first = float(closure_S().detach())
opt.step(closure_S)
last = float(closure_S().detach())
err = float((S.index_add(0, moved, offset.detach()) - S_true).abs().max())
print("three node positions: misfit %.3e -> %.3e, max distance from the true coordinates %.3e (of a spacing of %.3e)" % (first, last, err, h2 ** 0.5))
assert last < 1e-3 * first
