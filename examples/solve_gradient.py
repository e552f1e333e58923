#!/usr/bin/env python3
"""Extension: gradients through a PREPARED solver.  The geometry of a small scattered cloud is prepared once in an ExpertSolver; the values
of several fields on it are then recovered from their target derivatives (plus one anchor value each) by gradient descent: every step
solves all fields on the prepared geometry (wlsqm.hip.differentiable_solve_many) and runs the adjoint of that solve backward — with the
stored solution operator (prepare_operator()) one batched GEMM with its transpose for the whole stack."""
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "python-wlsqm_amd"))
import wlsqm
import wlsqm.hip

dev = torch.device("cuda", 0)
rng = np.random.default_rng(4)
npoints, k, order, nfields = 400, 16, 2, 3
S = torch.from_numpy(rng.uniform(0.0, 1.0, (npoints, 2))).to(dev)
truth = torch.stack([torch.sin((1.0 + 0.5 * r) * np.pi * S[:, 0]) * torch.cos(np.pi * S[:, 1]) for r in range(nfields)])

hoods = wlsqm.hip.knn(S, k).long()                                # (npoints, k), on the device
solver = wlsqm.ExpertSolver(dimension=2, nk=np.full(npoints, k, np.int32), order=np.full(npoints, order, np.int32),
                            knowns=np.zeros(npoints, np.int64), weighting_method=np.full(npoints, wlsqm.WEIGHT_CENTER, np.int32))
solver.prepare_device(S, S[hoods].contiguous())                   # the geometry: once
solver.prepare_operator()                                         # the stored solution operator: forward and adjoint are GEMMs
no = wlsqm.number_of_dofs(2, order)
fi0 = torch.zeros((nfields, npoints, no), dtype=torch.float64, device=dev)
grad_cols = [wlsqm.i2_X, wlsqm.i2_Y]


def fitted_gradients(F):                                          # F (nfields, npoints) -> (nfields, npoints, 2)
    return wlsqm.hip.differentiable_solve_many(solver, F[:, hoods], fi0)[:, :, grad_cols]


target = fitted_gradients(truth).detach()                         # what is observed: the fitted gradients of the true fields
F = torch.zeros((nfields, npoints), dtype=torch.float64, device=dev, requires_grad=True)
opt = torch.optim.Adam([F], lr=0.05)
for step in range(401):
    opt.zero_grad()
    mismatch = ((fitted_gradients(F) - target) ** 2).mean()
    loss = mismatch + ((F[:, 0] - truth[:, 0]) ** 2).sum()        # a gradient fixes a field up to a constant: anchor one value each
    loss.backward()                                               # the solve's adjoint, then torch's scatter of dL/dfk into dL/dF
    opt.step()
    if step % 50 == 0:
        err = (F.detach() - truth).abs().max()
        print("step %3d  loss %.3e  max |F - truth| = %.3e  (backward: %s)" % (step, loss.item(), err.item(), wlsqm.hip.last_kernel()))
