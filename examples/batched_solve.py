"""Many small dense systems on the GPU: 10^6 independent 6 x 6 solves, device-resident, then factor once / solve many.

    python examples/batched_solve.py

The arrays keep the layout of wlsqm.utils.lapackdrivers (Fortran order: A (n, n, count), b (n, count)), so the same
data can go through the host-array API (lapackdrivers.mgeneral & co.) or stay on the device (wlsqm.hip.*_batched).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "python-wlsqm_amd"))

import torch  # noqa: E402

from wlsqm import hip as H  # noqa: E402
from wlsqm.utils import lapackdrivers as L  # noqa: E402


def main():
    rng = np.random.default_rng(0)
    n, count = 6, 10 ** 6
    A_host = np.asfortranarray(rng.random((n, n, count)) + n * np.eye(n)[:, :, None])
    b_host = np.asfortranarray(rng.random((n, count)))

    # 1. one launch: LU with partial pivoting + solve of every system, in place on the device
    A = torch.from_numpy(A_host).cuda()
    b = torch.from_numpy(b_host).cuda()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ipiv, info = H.gesv_batched(A, b)
    e1.record()
    torch.cuda.synchronize()
    x = b.cpu().numpy()
    r = np.einsum("ijk,jk->ik", A_host, x) - b_host
    print("gesv: %d systems of %d x %d in %.3f ms, singular: %d, max residual %.2e"
          % (count, n, n, e0.elapsed_time(e1), int((info != 0).sum()), np.abs(r).max()))

    # 2. factor one matrix once, then solve for many right-hand sides with the same factor (A (n, n, 1))
    M = torch.from_numpy(np.asfortranarray(A_host[:, :, :1])).cuda()
    piv, _ = H.getrf_batched(M)
    rhs = torch.from_numpy(np.asfortranarray(rng.random((n, count)))).cuda()
    rhs0 = rhs.cpu().numpy()
    H.getrs_batched(M, piv, rhs)
    torch.cuda.synchronize()
    r = A_host[:, :, 0] @ rhs.cpu().numpy() - rhs0
    print("getrs: %d right-hand sides with one factor, max residual %.2e" % (count, np.abs(r).max()))

    # 3. the same through the reference's host API (numpy arrays in and out)
    A2, b2 = A_host[:, :, :1000].copy(order="F"), b_host[:, :1000].copy(order="F")
    L.mgeneral(A2, b2)
    print("lapackdrivers.mgeneral agrees with the device path bit for bit:", np.array_equal(b2, x[:, :1000]))


if __name__ == "__main__":
    main()
