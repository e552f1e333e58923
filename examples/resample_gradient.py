#!/usr/bin/env python3
"""Extension: gradients through fit AND resampling.  A field on a scattered cloud is observed only at sensor positions that are not cloud
points.  The cloud values are recovered by gradient descent on the misfit at the sensors: every step fits the cloud on the prepared
geometry (wlsqm.hip.differentiable_solve), evaluates the fitted models at the sensors through an interpolation plan
(wlsqm.hip.differentiable_evaluate), and runs both adjoints backward — the plan's is one deterministic gather over its inverted index, no
atomics, so two runs of this script print the same digits."""
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "python-wlsqm_amd"))
import wlsqm
import wlsqm.hip

dev = torch.device("cuda", 0)
rng = np.random.default_rng(4)
npoints, nsensors, k, order = 400, 1500, 16, 2
S = torch.from_numpy(rng.uniform(0.0, 1.0, (npoints, 2))).to(dev)
X = torch.from_numpy(rng.uniform(0.05, 0.95, (nsensors, 2))).to(dev)       # the sensors: off the cloud
truth = torch.sin(np.pi * S[:, 0]) * torch.cos(np.pi * S[:, 1])

hoods = wlsqm.hip.knn(S, k).long()                                # (npoints, k), on the device
solver = wlsqm.ExpertSolver(dimension=2, nk=np.full(npoints, k, np.int32), order=np.full(npoints, order, np.int32),
                            knowns=np.zeros(npoints, np.int64), weighting_method=np.full(npoints, wlsqm.WEIGHT_CENTER, np.int32))
solver.prepare_device(S, S[hoods].contiguous())                   # the geometry: once
plan = solver.interpolation_plan(X)                               # the sensors' models: searched once
plan.prepare_adjoint()                                            # the inverted index of the backward pass: once
fi0 = torch.zeros((npoints, wlsqm.number_of_dofs(2, order)), dtype=torch.float64, device=dev)


def at_sensors(F):                                                # F (npoints,) -> the fitted field at the sensors (nsensors,)
    fi = wlsqm.hip.differentiable_solve(solver, F[hoods], fi0)
    return wlsqm.hip.differentiable_evaluate(plan, fi, 0)


observed = at_sensors(truth).detach()
F = torch.zeros(npoints, dtype=torch.float64, device=dev, requires_grad=True)
opt = torch.optim.Adam([F], lr=0.05)
for step in range(301):
    opt.zero_grad()
    loss = ((at_sensors(F) - observed) ** 2).mean()
    loss.backward()                                               # the plan's adjoint, the solve's adjoint, torch's scatter into dL/dF
    opt.step()
    if step % 50 == 0:
        err = (F.detach() - truth).abs().max()
        print("step %3d  misfit %.3e  max |F - truth| = %.3e" % (step, loss.item(), err.item()))
