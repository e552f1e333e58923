"""What the tests of the device-resident API share: a host tensor that passes for a device tensor (the argument checks run before
anything touches the GPU), the one-liners of the GPU tests that move arrays and compare bits, and the module-scoped fixtures of the
adversarial GPU modules (imported by name into the module that uses them)."""
import numpy as np
import pytest


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


def same_bits(a, b):
    """numpy arrays bit for bit, any NaN standing for any NaN."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


@pytest.fixture(scope="module")
def wlsqm():
    import wlsqm as W
    from wlsqm import _binding
    assert _binding.lib().wlsqm_hip_device_count() >= 1, "no HIP device: the GPU tests need a real MI355X"
    return W


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O
