#!/usr/bin/env python3
"""Extension: gradients with respect to the COORDINATES of a fit.  A few points of a small scattered cloud are moved so that the derivative
d/dx fitted at one probe point matches a target value: every step runs the index-based fit forward
(wlsqm.hip.differentiable_fit_cloud(..., geometry=True)) and the geometry adjoint backward, which carries dL/dfi_out to the point table S
(one kernel, then two index_add_ into dL/dS).  The data are carried by the points (a quantity that particles take along): F stays as
sampled on the starting cloud, only the coordinates change."""
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "python-wlsqm_amd"))
import wlsqm
import wlsqm.hip

dev = torch.device("cuda", 0)
rng = np.random.default_rng(5)
npoints, k, order = 200, 12, 2
S0 = torch.from_numpy(rng.uniform(0.0, 1.0, (npoints, 2))).to(dev)
field = lambda P: torch.sin(3.0 * P[:, 0]) * torch.cos(2.0 * P[:, 1])

hoods = wlsqm.hip.knn(S0, k)                                      # the neighbour lists stay those of the starting cloud
nk = torch.full((npoints,), k, dtype=torch.int32, device=dev)
knowns = torch.zeros((npoints,), dtype=torch.int64, device=dev)
wm = torch.full((npoints,), wlsqm.WEIGHT_CENTER, dtype=torch.int32, device=dev)
F = field(S0)                                                     # carried along: not re-sampled when a point moves
fi0 = torch.zeros((npoints, wlsqm.number_of_dofs(2, order)), dtype=torch.float64, device=dev)

probe = 0
movable = hoods[probe, :4].long()                                 # the probe's four nearest neighbours may move
mask = torch.zeros((npoints, 1), dtype=torch.float64, device=dev)
mask[movable] = 1.0
shift = torch.zeros((npoints, 2), dtype=torch.float64, device=dev, requires_grad=True)


def fitted_dx(shift):
    S = S0 + mask * shift
    fi = wlsqm.hip.differentiable_fit_cloud(2, order, S, F, hoods, fi0, nk, knowns, wm, geometry=True)
    return fi[probe, wlsqm.i2_X]


start = fitted_dx(shift).item()
target = start + 0.05                                             # ask for a slightly different fitted derivative at the probe
opt = torch.optim.Adam([shift], lr=2e-3)
for step in range(201):
    opt.zero_grad()
    loss = (fitted_dx(shift) - target) ** 2
    loss.backward()                                               # geometry adjoint kernel + index_add_ into dL/dS
    opt.step()
    if step % 25 == 0:
        print("step %3d  fitted d/dx %.6f  target %.6f  largest move %.3e"
              % (step, fitted_dx(shift).item(), target, (mask * shift).detach().abs().max().item()))
