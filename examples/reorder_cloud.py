#!/usr/bin/env python3
"""A cloud that comes in random order, as a mesh generator or a file leaves it: wlsqm.hip.SpatialOrder puts it in Morton order on the
device, the neighbour search, the Laplacian of the local fits (wlsqm.hip.StencilOperator) and a large backward-Euler step
(I - nu dt Lap_h) u_new = u_old with wlsqm.hip.BlockJacobi(16) run on the ordered cloud, and order.restore brings the solution back to
the numbering the caller knows.  The last lines solve the same system on the cloud as given: the blocks of 16 consecutive rows hold no
neighbours there, and every gather of the solver misses L2."""
import os, sys, time
import numpy as np
import torch
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "python-wlsqm_amd"))
import synth
import wlsqm
import wlsqm.hip

n, nk, order_, tau = 200_000, 24, 2, 1.0
dev = torch.device("cuda", 0)
S_given = torch.from_numpy(np.ascontiguousarray(synth.halton(n, 2)[np.random.default_rng(0).permutation(n)])).to(dev)
u_given = torch.sin(np.pi * S_given[:, 0]) * torch.sin(np.pi * S_given[:, 1])
h2 = 1.0 / n


def laplacian(S):
    hoods = wlsqm.hip.knn(S, nk)
    nk_d = torch.full((n,), nk, dtype=torch.int32, device=dev)
    knowns = torch.full((n,), wlsqm.b2_F, dtype=torch.int64, device=dev)
    wm = torch.full((n,), wlsqm.WEIGHT_CENTER, dtype=torch.int32, device=dev)
    return wlsqm.hip.StencilOperator(2, order_, S, hoods, nk_d, knowns, wm, wlsqm.hip.stencil_rows(2, order_, "laplacian", device=dev))


def solve(op, b):
    solver = wlsqm.hip.StencilSolver(op, diag=1.0, scale=-tau * h2, preconditioner=wlsqm.hip.BlockJacobi(16), method="bicgstab2")
    x = torch.zeros_like(b)
    solver.solve(b, x, rtol=1e-10, maxiter=4)                       # warm-up
    x.zero_()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    info = solver.solve(b, x, rtol=1e-10, maxiter=4000, check_every=16)
    torch.cuda.synchronize()
    return x, info, (time.perf_counter() - t0) * 1e3


torch.cuda.synchronize(); t0 = time.perf_counter()
order = wlsqm.hip.SpatialOrder(S_given)
torch.cuda.synchronize()
print("SpatialOrder of %d points in %dD: %.2f ms; box %s .. %s, %d bits per axis" % (n, order.dimension, (time.perf_counter() - t0) * 1e3,
                                                                                      order.lo, order.hi, order.bits))
S = order.take(S_given).contiguous()                                 # the cloud in the new order; fields follow with order.take
x, info, ms = solve(laplacian(S), order.take(u_given))
u_new = order.restore(x)                                             # back in the caller's numbering
print("ordered:  status %d after %4d iterations, %.2f ms" % (info.status, info.iterations, ms))

# a finished operator of the cloud as given can be renumbered too (P A P^T; order.hoods does the same for neighbour lists)
lap_given = laplacian(S_given)
x2, info2, ms2 = solve(order.operator(lap_given), order.take(u_given))
print("order.operator of the operator as given: status %d after %4d iterations, %.2f ms; against the ordered cloud's solution %.2e"
      % (info2.status, info2.iterations, ms2, float((x2 - x).abs().max())))

x_given, info_given, ms_given = solve(lap_given, u_given)
print("as given: status %d after %4d iterations, %.2f ms; the two solutions differ by %.2e"
      % (info_given.status, info_given.iterations, ms_given, float((x_given - u_new).abs().max())))
