"""Interpolation plans (wlsqm.hip.InterpolationPlan, ExpertSolver.interpolation_plan): what can be checked without a GPU."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLAN_FUNCTIONS = ("create", "create_expert", "info", "export", "eval_device", "eval_expert", "destroy")


def test_header_declares_the_plan_entry_points():
    hdr = open(os.path.join(ROOT, "include", "wlsqm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"typedef\s+struct\s+wlsqm_interp_plan\s+wlsqm_interp_plan\s*;", hdr)
    for name in PLAN_FUNCTIONS:
        assert re.search(r"\bint\s+wlsqm_hip_interp_plan_%s\s*\(" % name, hdr), name
    # the coefficient-independent calls take device pointers and a stream; the evaluation takes the diffs by host array
    assert re.search(r"wlsqm_hip_interp_plan_eval_device\s*\([^;]*const\s+int32_t\s*\*\s*diffs\s*,\s*int\s+ndiff", hdr)


def test_library_exports_the_plan_entry_points():
    import ctypes as C
    from wlsqm import _binding
    lib = C.CDLL(_binding.LIB_PATH)
    for name in PLAN_FUNCTIONS:
        assert hasattr(lib, "wlsqm_hip_interp_plan_" + name), name


def test_python_surface():
    import wlsqm
    import wlsqm.hip as whip
    assert "InterpolationPlan" in whip.__all__
    sig = inspect.signature(whip.InterpolationPlan.__init__)
    assert list(sig.parameters) == ["self", "xi", "order", "x", "mode", "r", "I", "stream"]
    assert sig.parameters["mode"].default == "nearest" and sig.parameters["r"].default is None
    sig = inspect.signature(wlsqm.ExpertSolver.interpolation_plan)
    assert list(sig.parameters) == ["self", "x", "mode", "r", "I", "stream"]
    sig = inspect.signature(whip.InterpolationPlan.evaluate)
    assert list(sig.parameters) == ["self", "diff", "fi", "out", "stream"] and sig.parameters["diff"].default == 0
    for name in ("I", "lists", "memory_used", "close"):             # (nx, mode and r are set by the constructor)
        assert hasattr(whip.InterpolationPlan, name), name


def test_argument_checks_that_need_no_device():
    torch = pytest.importorskip("torch")
    import wlsqm.hip as whip
    xi = torch.zeros((10, 2), dtype=torch.float64)
    x = torch.zeros((5, 2), dtype=torch.float64)
    with pytest.raises(ValueError, match="mode must be one of"):
        whip.InterpolationPlan(xi, 2, x, mode="linear")
    with pytest.raises(ValueError, match="r must be specified"):
        whip.InterpolationPlan(xi, 2, x, mode="continuous")
    with pytest.raises(ValueError, match="r must be positive"):
        whip.InterpolationPlan(xi, 2, x, mode="continuous", r=0.0)
    with pytest.raises(ValueError, match="nearest"):
        whip.InterpolationPlan(xi, 2, x, mode="continuous", r=0.1, I=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError, match="dtype mismatch"):
        whip.InterpolationPlan(xi, 2, x.float())
    with pytest.raises(ValueError, match="device"):
        whip.InterpolationPlan(xi, 2, x)                         # float64, but a host tensor
    with pytest.raises(ValueError, match="device"):
        whip.InterpolationPlan(xi, 2, np.zeros((5, 2)))           # the standalone plan takes device tensors only
    # the diff list is checked before anything touches the plan: a sequence longer than the 35 DOFs of 3D order 4
    with pytest.raises(ValueError, match="at most 35"):
        whip._diff_list(list(range(36)))
    assert whip._diff_list(3) == ([3], True) and whip._diff_list([0, 2, 2]) == ([0, 2, 2], False)
    assert whip._diff_list(range(35))[0] == list(range(35))
    with pytest.raises(ValueError):
        whip._diff_list(None)
    plan = whip.InterpolationPlan.__new__(whip.InterpolationPlan)      # no device-side state: evaluate() still checks diff first
    plan._handle = None
    with pytest.raises(ValueError, match="at most 35"):
        plan.evaluate(list(range(36)))
    with pytest.raises(RuntimeError, match="closed"):
        plan.evaluate(0)
    plan.close()
    plan.close()
