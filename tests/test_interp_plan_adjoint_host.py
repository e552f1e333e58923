"""The adjoint of interpolation plans (InterpolationPlan.evaluate_adjoint, wlsqm.hip.differentiable_evaluate; csrc/interp_plan.hip,
DESIGN.md section 14): what can be checked without a GPU — the C and Python surface, the argument checks that need no device, and the
numpy reference of tests/_interp_adjoint_ref.py against its own forward, which pins the reference before it judges the kernel."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import _interp_adjoint_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADJOINT_FUNCTIONS = ("prepare_adjoint", "adjoint_info", "export_transposed", "eval_adjoint_device")


def test_header_declares_the_adjoint_entry_points():
    hdr = open(os.path.join(ROOT, "include", "wlsqm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ADJOINT_FUNCTIONS:
        assert re.search(r"\bint\s+wlsqm_hip_interp_plan_%s\s*\(" % name, hdr), name
    m = re.search(r"\bint\s+wlsqm_hip_interp_plan_eval_adjoint_device\s*\(([^;]*)\)\s*;", hdr)
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert args == ["wlsqm_interp_plan* plan", "void* stream", "int64_t nfields", "const int32_t* diffs", "int ndiff",
                    "const double* g_dev", "int64_t g_stride_field", "int64_t g_stride_diff", "double* grad_fi_dev",
                    "int64_t gfi_stride_field", "int64_t gfi_stride_model", "int ncols"]
    assert re.search(r"wlsqm_hip_interp_plan_prepare_adjoint\s*\(\s*wlsqm_interp_plan\s*\*\s*plan\s*,\s*void\s*\*\s*stream\s*,\s*int\s*\*\s*built\s*\)", hdr)
    assert re.search(r"wlsqm_hip_interp_plan_adjoint_info\s*\([^;]*int64_t\s*\*\s*nentries\s*,\s*int64_t\s*\*\s*max_len\s*,\s*int64_t\s*\*\s*nlong\s*,"
                     r"\s*int32_t\s*\*\s*threshold\s*\)", hdr)


def test_library_exports_the_adjoint_entry_points():
    from wlsqm import _binding
    lib = C.CDLL(_binding.LIB_PATH)
    for name in ADJOINT_FUNCTIONS:
        assert hasattr(lib, "wlsqm_hip_interp_plan_" + name), name


def test_python_surface():
    import wlsqm
    import wlsqm.hip as whip
    assert "differentiable_evaluate" in whip.__all__ and not hasattr(wlsqm, "differentiable_evaluate")
    P = whip.InterpolationPlan
    assert list(inspect.signature(P.prepare_adjoint).parameters) == ["self", "stream"]
    assert inspect.signature(P.prepare_adjoint).parameters["stream"].default is None
    assert list(inspect.signature(P.adjoint_info).parameters) == ["self"]
    assert list(inspect.signature(P.transposed_lists).parameters) == ["self"]
    sig = inspect.signature(P.evaluate_adjoint)
    assert list(sig.parameters) == ["self", "g", "diff", "grad_fi", "ncols", "stream"]
    assert sig.parameters["diff"].default == 0
    assert all(sig.parameters[p].default is None for p in ("grad_fi", "ncols", "stream"))
    sig = inspect.signature(whip.differentiable_evaluate)
    assert list(sig.parameters) == ["plan", "fi", "diff", "stream"]
    assert sig.parameters["diff"].default == 0 and sig.parameters["stream"].default is None
    # evaluate itself stays as it is
    assert list(inspect.signature(P.evaluate).parameters) == ["self", "diff", "fi", "out", "stream"]


def test_argument_checks_that_need_no_device():
    torch = pytest.importorskip("torch")
    import wlsqm.hip as whip
    plan = whip.InterpolationPlan.__new__(whip.InterpolationPlan)      # no device-side state
    plan._handle = None
    g = torch.zeros(5, dtype=torch.float64)
    # the diff list is checked first, then that g is a float64 device tensor, then the plan
    with pytest.raises(ValueError, match="at most 35"):
        plan.evaluate_adjoint(g, list(range(36)))
    with pytest.raises(ValueError, match="device"):
        plan.evaluate_adjoint(g)
    with pytest.raises(ValueError, match="device"):
        plan.evaluate_adjoint(np.zeros(5))
    with pytest.raises(ValueError, match="dtype mismatch"):
        plan.evaluate_adjoint(g.float())
    for call in (plan.prepare_adjoint, plan.adjoint_info, plan.transposed_lists):
        with pytest.raises(RuntimeError, match="closed"):
            call()
    with pytest.raises(ValueError, match="explicitly"):
        whip.differentiable_evaluate(plan, None)
    plan._geometry_requires_grad = True
    with pytest.raises(ValueError, match="not differentiable"):
        whip.differentiable_evaluate(plan, g)
    plan.close()


def _geometry(dim, mode, rng):
    nmodels, nx = 60, 157
    xi = rng.uniform(0.0, 1.0, size=(nmodels, dim))
    xi[-5:] += 10.0                                                  # models that no point uses
    x = rng.uniform(-0.1, 1.1, size=(nx, dim))
    top = 4 if dim < 3 else 3
    order = rng.integers(0, top + 1, size=nmodels)
    kw = {}
    if mode == "nearest":
        d2 = ((x[:, None, :] - xi[None, :, :]) ** 2).sum(axis=2)
        I = d2.argmin(axis=1)
        I[::17] = -1
        I[5::23] = nmodels
        kw["I"] = I
    else:
        r = {1: 0.05, 2: 0.2, 3: 0.35}[dim]
        d2 = ((x[:, None, :] - xi[None, :, :]) ** 2).sum(axis=2)
        inside = d2 <= r * r
        off = np.concatenate([[0], np.cumsum(inside.sum(axis=1))])
        idx = np.nonzero(inside)[1]
        assert (np.diff(off) == 0).any() and (np.diff(off) > 1).any()
        kw["lists"], kw["r"] = (off, idx), r
    return xi, order, x, kw


@pytest.mark.parametrize("mode", ["nearest", "continuous"])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_reference_adjoint_is_the_adjoint_of_the_reference_forward(dim, mode):
    """<forward(fi), g> == <fi, adjoint(g)>: both sides are sums of the same terms, so they differ by no more than
    sum over the elements of (128 + 4 (n + len_max)) eps A |fi| (tests/_interp_adjoint_ref.bound), once for either side."""
    rng = np.random.default_rng(100 + 10 * dim + (mode == "continuous"))
    xi, order, x, kw = _geometry(dim, mode, rng)
    ncols = R.NDOF[dim][4 if dim < 3 else 3]
    diffs = [int(d) for d in rng.permutation(ncols)] + [2 % ncols, ncols + 4, -1]        # all of them, a repeat, two that nobody has
    fi = rng.standard_normal((len(order), ncols))
    g = rng.standard_normal((len(diffs), x.shape[0]))
    out = R.forward(dim, xi, order, x, fi, diffs, **kw)
    grad, A, n, len_max = R.adjoint(dim, xi, order, x, g, diffs, ncols, **kw)
    assert (len_max == 0) == (mode == "nearest")
    no = np.array(R.NDOF[dim])[order]
    cols = np.arange(ncols)[None, :]
    assert (grad[cols >= no[:, None]] == 0.0).all() and (n[cols >= no[:, None]] == 0).all()
    assert (n.sum(axis=1) == 0).any() and (n > 0).any()                  # a model nobody uses, and work to do
    lhs, rhs = float((out * g).sum()), float((fi * grad).sum())
    tol = 2.0 * float((R.bound(A, n, len_max) * np.abs(fi)).sum())
    print("dim %d %s: |<Jf, g> - <f, J'g>| = %.3e, bound %.3e" % (dim, mode, abs(lhs - rhs), tol))
    assert tol > 0.0 and abs(lhs - rhs) <= tol
    # g at the points that do not depend on fi is not read
    dead = np.ones(x.shape[0], bool)
    dead[R.entries(dim, xi, x, len(order), kw.get("I"), kw.get("lists"), kw.get("r"))[0]] = False
    assert dead.any()
    g_nan = g.copy()
    g_nan[:, dead] = np.nan
    assert np.array_equal(R.adjoint(dim, xi, order, x, g_nan, diffs, ncols, **kw)[0], grad)
