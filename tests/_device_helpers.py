"""What the tests of the device-resident API share: a host tensor that passes for a device tensor (the argument checks run before
anything touches the GPU), and the three one-liners of the GPU tests that compare bits."""
import numpy as np


class OnDevice:
    """A host tensor that says it lives on the device: the argument checks run before anything touches the GPU."""
    is_cuda = True

    def __init__(self, t):
        self._t = t

    def __getattr__(self, name):
        return getattr(self._t, name)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nan(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def bits(t):
    import torch
    return t.contiguous().view(torch.int64)
