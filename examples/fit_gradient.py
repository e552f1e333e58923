#!/usr/bin/env python3
"""Extension: a fit inside a differentiated computation.  The values of a field on a small scattered cloud are recovered from its
fitted GRADIENT alone (plus the value at one anchor point) by gradient descent on the mismatch: every step runs the index-based fit
forward (wlsqm.hip.differentiable_fit_cloud) and its adjoint backward — one kernel each, no sensitivities are ever formed."""
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "python-wlsqm_amd"))
import wlsqm
import wlsqm.hip

dev = torch.device("cuda", 0)
rng = np.random.default_rng(3)
npoints, k, order = 400, 16, 2
S = torch.from_numpy(rng.uniform(0.0, 1.0, (npoints, 2))).to(dev)
truth = torch.sin(np.pi * S[:, 0]) * torch.cos(np.pi * S[:, 1])

hoods = wlsqm.hip.knn(S, k)                                       # (npoints, k) int32, on the device
nk = torch.full((npoints,), k, dtype=torch.int32, device=dev)
knowns = torch.zeros((npoints,), dtype=torch.int64, device=dev)   # every DOF is fitted, the value included
wm = torch.full((npoints,), wlsqm.WEIGHT_CENTER, dtype=torch.int32, device=dev)
no = wlsqm.number_of_dofs(2, order)
fi0 = torch.zeros((npoints, no), dtype=torch.float64, device=dev)
grad_cols = [wlsqm.i2_X, wlsqm.i2_Y]


def fitted_gradient(F):
    return wlsqm.hip.differentiable_fit_cloud(2, order, S, F, hoods, fi0, nk, knowns, wm)[:, grad_cols]


target = fitted_gradient(truth).detach()                          # what is observed: the fitted gradient of the true field
F = torch.zeros(npoints, dtype=torch.float64, device=dev, requires_grad=True)
opt = torch.optim.Adam([F], lr=0.05)
for step in range(401):
    opt.zero_grad()
    mismatch = ((fitted_gradient(F) - target) ** 2).mean()
    loss = mismatch + (F[0] - truth[0]) ** 2                      # a gradient fixes a field up to a constant: anchor one value
    loss.backward()                                               # the adjoint kernel + one index_add_ into dL/dF
    opt.step()
    if step % 50 == 0:
        err = (F.detach() - truth).abs().max()
        print("step %3d  loss %.3e  max |F - truth| = %.3e" % (step, loss.item(), err.item()))
