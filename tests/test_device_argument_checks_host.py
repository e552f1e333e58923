"""The argument checks of the device-resident API, pinned: every row of the table below is one call that violates exactly one
precondition of a public entry point of wlsqm.hip or of ExpertSolver's device-resident methods, and
tests/golden/device_argument_checks.json holds, per row, the exception type and the full message that the call raised BEFORE the
checks were gathered into shared helpers (recorded at commit cec4e7c by ``python tests/test_device_argument_checks_host.py
--record``; record it from that commit or an ancestor only, never from the code under test).  The test asserts equality of both.

The calls are built on the OnDevice stub (tests/_device_helpers.py): host tensors that say they live on the device, so the checks
run and fail before anything reaches the GPU or the library.  wlsqm._binding.lib is replaced for the duration of a row by a
function that raises: a row that gets as far as the library is not a validation row, and fails.

Left out, and why:
  * differentiable_evaluate(plan, fi, diff=None): it used to fail in ``int(None)``, a TypeError whose text belongs to the Python
    version; the wrapper now normalises `diff` through _diff_list as evaluate does, which says "diff cannot be None".
  * rows whose message would embed a tensor's repr or an address: there are none, every message is made of names, counts, dtypes
    and shape tuples.
  * checks that sit behind the first use of a real device (the allocations of the adjoints' outputs on the device of g, the stream
    lookup of a tensor without a device index, InterpolationPlan's per-case order scan): their rows pass the outputs in and name
    device 0 and stream 0 where that lets the check run, and are absent where it does not.
"""
import json
import os
import sys

import numpy as np
import pytest

from _device_helpers import OnDevice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "device_argument_checks.json")


class _ReachedTheLibrary(BaseException):
    pass


def _no_library():
    raise _ReachedTheLibrary()


class OnDevice0(OnDevice):
    """OnDevice that also names its device (cuda:0), for the checks that come after the stream and device lookup."""

    @property
    def device(self):
        import torch
        return torch.device("cuda", 0)


def _other_dtype(t):
    import torch
    return t.to({torch.float64: torch.float32, torch.int32: torch.int64, torch.int64: torch.int32}[t.dtype])


# one violation each: host tensor in, argument out (wrapped by D unless the violation is "not on the device")
KINDS = {
    "dtype": lambda t, D: D(_other_dtype(t)),
    "rank": lambda t, D: D(t[0] if t.dim() > 1 else t[:, None]),
    "host": lambda t, D: t,
    "rows": lambda t, D: D(t[:-1]),
    "contiguous": lambda t, D: D(t.repeat_interleave(2, dim=-1)[..., ::2]),
    "columns": lambda t, D: D(t[..., :-1]),
    "slots": lambda t, D: D(t[:, :-1]),
    "stack": lambda t, D: D(t[:-1]),
    "solver_rows": lambda t, D: D(t[..., :-1, :]),
}

CHECK = ("dtype", "rank", "host")


def _wrap(d, D=OnDevice):
    return {k: (D(v) if hasattr(v, "data_ptr") else v) for k, v in d.items()}


def _dense(dim=2, no=6, n=4, K=7):
    import torch
    g = torch.Generator().manual_seed(0)
    f64 = torch.float64
    xk = torch.rand((n, K, dim) if dim > 1 else (n, K), dtype=f64, generator=g)
    xi = torch.zeros((n, dim) if dim > 1 else (n,), dtype=f64)
    return dict(xk=xk, fk=torch.rand((n, K), dtype=f64, generator=g), nk=torch.full((n,), K, dtype=torch.int32), xi=xi,
                fi=torch.zeros((n, no), dtype=f64), knowns=torch.zeros((n,), dtype=torch.int64),
                weighting_method=torch.full((n,), 2, dtype=torch.int32))


def _cloud(dim=2, no=6, npoints=10, n=4, K=7):
    import torch
    f64 = torch.float64
    return dict(S=torch.rand((npoints, dim), dtype=f64, generator=torch.Generator().manual_seed(1)), F=torch.ones((npoints,), dtype=f64),
                hoods=torch.ones((n, K), dtype=torch.int32), fi=torch.zeros((n, no), dtype=f64), nk=torch.full((n,), K, dtype=torch.int32),
                knowns=torch.zeros((n,), dtype=torch.int64), weighting_method=torch.full((n,), 2, dtype=torch.int32))


def _solver(ready=True, n=4, max_nk=8, no=6):
    """An ExpertSolver shell without device state: what the argument checks look at."""
    from wlsqm.fitter.expert import ExpertSolver
    s = ExpertSolver.__new__(ExpertSolver)
    s._handle = None; s._tree = None; s._tree_points = None
    s.ready, s.ncases, s._max_nk, s._max_no, s._device, s.dimension = ready, n, max_nk, no, 0, 2
    s.order = np.full(n, 2, np.int32)
    return s


def _plan(nx=5, nmodels=10, max_no=6):
    """An InterpolationPlan shell: a handle that is never handed to the library, and that close() only forgets."""
    import torch
    import wlsqm.hip as h

    class Shell(h.InterpolationPlan):
        def close(self):
            self._handle = None

    p = Shell.__new__(Shell)
    p._handle, p._solver, p._max_no, p._geometry_requires_grad = 1, None, max_no, False
    p.dimension, p.nmodels, p.nx, p._device, p._I, p.mode, p.r = 2, nmodels, nx, torch.device("cpu"), None, "nearest", None
    return p


def build_rows():
    """[(id, thunk)]: id = entry point / argument / violation."""
    import torch
    import wlsqm.hip as h
    f64 = torch.float64
    D, D0 = OnDevice, OnDevice0
    rows = []

    def add(rid, fn, *args, **kw):
        assert rid not in dict(rows), rid
        rows.append((rid, lambda: fn(*args, **kw)))

    def sweep(entry, fn, raw, spec, extra=None, wrap=D):
        """One row per (argument, kind) of `spec`: the base arguments `raw` with that one argument spoilt."""
        for name, kinds in spec:
            for kind in kinds:
                a = dict(_wrap(raw, wrap), **(extra or {}))
                a[name] = KINDS[kind](raw[name], wrap)
                add("%s/%s/%s" % (entry, name, kind), fn, **a)

    # ---- fit_many_device ----
    d = _dense()
    many = lambda **a: h.fit_many_device(2, 2, **a)
    sweep("fit_many_device", many, d, [("nk", CHECK), ("knowns", CHECK + ("rows",)), ("weighting_method", CHECK + ("rows",)),
                                        ("fk", CHECK + ("rows",)), ("fi", CHECK + ("rows", "contiguous", "columns")),
                                        ("xk", CHECK + ("rows", "contiguous", "columns", "slots")),
                                        ("xi", CHECK + ("rows", "contiguous", "columns"))])
    sens = torch.zeros((4, 7, 6), dtype=f64)
    sweep("fit_many_device", many, dict(d, sens=sens), [("sens", CHECK + ("rows", "contiguous", "columns", "slots"))])
    d1 = _dense(dim=1, no=3)
    sweep("fit_many_device[1D]", lambda **a: h.fit_many_device(1, 2, **a), d1, [("xk", ("rank", "dtype")), ("xi", ("rank", "dtype"))])
    add("fit_many_device/dimension/value", h.fit_many_device, 4, 2, **_wrap(d))
    add("fit_many_device/order/value", h.fit_many_device, 2, 5, **_wrap(d))
    order_t = torch.full((4,), 2, dtype=torch.int32)
    wide = dict(d, fi=torch.zeros((4, 15), dtype=f64))
    sweep("fit_many_device[order tensor]", lambda order, **a: h.fit_many_device(2, order, **a), dict(wide, order=order_t),
          [("order", ("dtype", "rank", "rows")), ("fi", ("columns",)), ("nk", ("dtype",))])
    add("fit_many_device[order tensor]/case_index/excluded", h.fit_many_device, 2, D(order_t),
        **dict(_wrap(wide), case_index=D(torch.zeros(2, dtype=torch.int64))))
    add("fit_many_device[order tensor]/fi/max_order", h.fit_many_device, 2, D(order_t), **dict(_wrap(wide), max_order=5))
    ci = torch.zeros(2, dtype=torch.int64)
    sweep("fit_many_device", many, dict(d, case_index=ci), [("case_index", CHECK)], extra=dict(stream=0), wrap=D0)

    # ---- fit_cloud_device ----
    c = _cloud()
    pidx = torch.arange(4, dtype=torch.int32)
    cloud = lambda **a: h.fit_cloud_device(2, 2, **a)
    sweep("fit_cloud_device", cloud, c, [("F", CHECK + ("contiguous", "rows")), ("hoods", CHECK + ("contiguous",)),
                                         ("fi", CHECK + ("contiguous", "rows", "columns")), ("S", CHECK + ("contiguous",)),
                                         ("nk", CHECK + ("contiguous", "rows")), ("knowns", CHECK + ("contiguous", "rows")),
                                         ("weighting_method", CHECK + ("contiguous", "rows"))])
    sweep("fit_cloud_device", cloud, dict(c, point_index=pidx), [("point_index", CHECK + ("rows",))])
    add("fit_cloud_device/S/points", cloud, **dict(_wrap(c), S=D(c["S"][:3]), F=D(c["F"][:3])))
    add("fit_cloud_device/S/coordinates", cloud, **dict(_wrap(c), S=D(torch.zeros((10, 3), dtype=f64))))
    add("fit_cloud_device/order/value", h.fit_cloud_device, 2, 5, **_wrap(c))
    sweep("fit_cloud_device", cloud, dict(c, sens=sens), [("sens", CHECK + ("rows", "contiguous", "columns", "slots"))],
          extra=dict(stream=0), wrap=D0)
    c1 = dict(_cloud(), S=torch.rand((10,), dtype=f64, generator=torch.Generator().manual_seed(2)), fi=torch.zeros((4, 3), dtype=f64))
    sweep("fit_cloud_device[1D]", lambda **a: h.fit_cloud_device(1, 2, **a), c1, [("S", ("rank",))])

    # ---- fit_many_adjoint_device ----
    ad = {k: v for k, v in d.items() if k not in ("fk", "fi")}
    ad.update(g=torch.ones((4, 6), dtype=f64), grad_fk=torch.zeros((4, 7), dtype=f64), grad_fi=torch.zeros((4, 6), dtype=f64))
    madj = lambda **a: h.fit_many_adjoint_device(2, 2, **a)
    sweep("fit_many_adjoint_device", madj, ad, [("nk", CHECK), ("knowns", CHECK + ("rows",)), ("weighting_method", CHECK + ("rows",)),
                                                ("xk", CHECK + ("rows", "contiguous", "columns")),
                                                ("xi", CHECK + ("rows", "contiguous", "columns")),
                                                ("g", CHECK + ("rows", "contiguous", "columns")),
                                                ("grad_fk", CHECK + ("rows", "slots")),
                                                ("grad_fi", CHECK + ("rows", "contiguous", "columns"))])
    sweep("fit_many_adjoint_device[1D]", lambda **a: h.fit_many_adjoint_device(1, 1, **a),
          dict({k: v for k, v in d1.items() if k not in ("fk", "fi")}, g=torch.ones((4, 2), dtype=f64)),
          [("xk", ("rank",)), ("xi", ("rank",)), ("g", ("columns",))])
    add("fit_many_adjoint_device/order/tensor", h.fit_many_adjoint_device, 2, D(d["nk"]), **_wrap(ad))
    add("fit_many_adjoint_device/order/value", h.fit_many_adjoint_device, 2, 5, **_wrap(ad))
    d3 = _dense(dim=3, no=20)
    ad3 = dict({k: v for k, v in d3.items() if k not in ("fk", "fi")}, g=torch.ones((4, 20), dtype=f64))
    add("fit_many_adjoint_device/order/3D order 3", h.fit_many_adjoint_device, 3, 3, **_wrap(ad3))
    add("fit_many_adjoint_device/g/device", madj, **dict(_wrap(ad), g=D0(ad["g"])))
    add("fit_many_adjoint_device/xk/device", madj, **dict(_wrap(ad, D0), xk=D(ad["xk"])))
    sweep("fit_many_adjoint_device", madj, dict(ad, case_index=ci), [("case_index", CHECK)], extra=dict(stream=0), wrap=D0)

    # ---- fit_cloud_adjoint_device ----
    ac = {k: v for k, v in c.items() if k not in ("F", "fi")}
    ac.update(g=torch.ones((4, 6), dtype=f64), grad_F=torch.zeros((10,), dtype=f64), grad_fi=torch.zeros((4, 6), dtype=f64),
              slots=torch.zeros((4, 7), dtype=f64))
    cadj = lambda **a: h.fit_cloud_adjoint_device(2, 2, **a)
    sweep("fit_cloud_adjoint_device", cadj, ac, [("hoods", CHECK + ("contiguous",)), ("S", CHECK + ("contiguous",)),
                                                 ("nk", CHECK + ("contiguous", "rows")), ("knowns", CHECK + ("contiguous", "rows")),
                                                 ("weighting_method", CHECK + ("contiguous", "rows")),
                                                 ("g", CHECK + ("rows", "contiguous", "columns")),
                                                 ("slots", CHECK + ("rows", "contiguous", "columns")),
                                                 ("grad_fi", CHECK + ("rows", "contiguous", "columns")),
                                                 ("grad_F", CHECK + ("rows",))])
    sweep("fit_cloud_adjoint_device", cadj, dict(ac, point_index=pidx), [("point_index", CHECK + ("rows",))])
    add("fit_cloud_adjoint_device/S/points", cadj, **dict(_wrap(ac), S=D(ac["S"][:3]), grad_F=D(ac["grad_F"][:3])))
    add("fit_cloud_adjoint_device/S/coordinates", cadj, **dict(_wrap(ac), S=D(torch.zeros((10, 3), dtype=f64))))
    add("fit_cloud_adjoint_device/order/tensor", h.fit_cloud_adjoint_device, 2, D(c["nk"]), **_wrap(ac))
    add("fit_cloud_adjoint_device/order/value", h.fit_cloud_adjoint_device, 2, 5, **_wrap(ac))
    c3 = _cloud(dim=3, no=20)
    ac3 = dict({k: v for k, v in c3.items() if k not in ("F", "fi")}, g=torch.ones((4, 20), dtype=f64))
    add("fit_cloud_adjoint_device/order/3D order 3", h.fit_cloud_adjoint_device, 3, 3, **_wrap(ac3))
    add("fit_cloud_adjoint_device/g/device", cadj, **dict(_wrap(ac), g=D0(ac["g"])))
    add("fit_cloud_adjoint_device/S/device", cadj, **dict(_wrap(ac, D0), S=D(ac["S"])))
    sweep("fit_cloud_adjoint_device[1D]", lambda **a: h.fit_cloud_adjoint_device(1, 1, **a),
          dict(ac, S=c1["S"], g=torch.ones((4, 2), dtype=f64), grad_fi=torch.zeros((4, 2), dtype=f64)), [("S", ("rank",))])

    # ---- differentiable_fit_many / differentiable_fit_cloud ----
    dm = lambda **a: h.differentiable_fit_many(2, 2, **a)
    add("differentiable_fit_many/order/tensor", h.differentiable_fit_many, 2, D(d["nk"]), **_wrap(d))
    add("differentiable_fit_many/order/value", h.differentiable_fit_many, 2, 5, **_wrap(d))
    add("differentiable_fit_many/order/3D order 3", h.differentiable_fit_many, 3, 3, **_wrap(d3))
    add("differentiable_fit_many/xk/requires_grad", dm, **dict(_wrap(d), xk=D(d["xk"].clone().requires_grad_())))
    add("differentiable_fit_many/xi/requires_grad", dm, **dict(_wrap(d), xi=d["xi"].clone().requires_grad_()))
    # the checks of the forward reach through the wrapper (those that come before fk, which the wrapper detaches from its stub)
    sweep("differentiable_fit_many", dm, d, [("nk", ("dtype", "rank")), ("knowns", ("dtype",)), ("weighting_method", ("dtype",))])
    dc = lambda **a: h.differentiable_fit_cloud(2, 2, **a)
    add("differentiable_fit_cloud/order/tensor", h.differentiable_fit_cloud, 2, D(c["nk"]), **_wrap(c))
    add("differentiable_fit_cloud/order/value", h.differentiable_fit_cloud, 2, 5, **_wrap(c))
    add("differentiable_fit_cloud/order/3D order 3", h.differentiable_fit_cloud, 3, 3, **_wrap(c3))
    add("differentiable_fit_cloud/S/requires_grad", dc, **dict(_wrap(c), S=D(c["S"].clone().requires_grad_())))

    # ---- the prepared solver: solve_device, solve_many_device, their adjoints and the two autograd wrappers ----
    s, u = _solver(), _solver(ready=False)
    fk2, fi2 = torch.ones((4, 8), dtype=f64), torch.ones((4, 6), dtype=f64)
    fk3, fi3 = torch.ones((3, 4, 8), dtype=f64), torch.ones((3, 4, 6), dtype=f64)
    SOLVER = ("dtype", "rank", "host", "contiguous", "solver_rows", "columns")
    for entry, fn, ufn, raw in (("solve_device", s.solve_device, u.solve_device, dict(fk=fk2, fi=fi2)),
                                ("solve_many_device", s.solve_many_device, u.solve_many_device, dict(fk=fk3, fi=fi3)),
                                ("differentiable_solve", lambda **a: h.differentiable_solve(s, **a),
                                 lambda **a: h.differentiable_solve(u, **a), dict(fk=fk2, fi=fi2)),
                                ("differentiable_solve_many", lambda **a: h.differentiable_solve_many(s, **a),
                                 lambda **a: h.differentiable_solve_many(u, **a), dict(fk=fk3, fi=fi3))):
        many_ = raw["fk"].dim() == 3
        sweep(entry, fn, raw, [("fk", SOLVER + (("stack",) if many_ else ())), ("fi", SOLVER + (("stack",) if many_ else ()))])
        if many_:
            add(entry + "/fk/empty stack", fn, fk=D(raw["fk"][:0]), fi=D(raw["fi"][:0]))
        add(entry + "/solver/not ready", ufn, **_wrap(raw))
    gk2, gk3 = torch.zeros((4, 8), dtype=f64), torch.zeros((3, 4, 8), dtype=f64)
    for entry, fn, ufn, raw in (("solve_adjoint_device", s.solve_adjoint_device, u.solve_adjoint_device,
                                 dict(g=fi2, grad_fk=gk2, grad_fi=fi2.clone())),
                                ("solve_many_adjoint_device", s.solve_many_adjoint_device, u.solve_many_adjoint_device,
                                 dict(g=fi3, grad_fk=gk3, grad_fi=fi3.clone()))):
        many_ = raw["g"].dim() == 3
        st = ("stack",) if many_ else ()
        sweep(entry, fn, raw, [("g", SOLVER + st), ("grad_fk", SOLVER + st), ("grad_fi", SOLVER + st)])
        sweep(entry + "[grad_fi=False]", fn, dict(g=raw["g"], grad_fk=raw["grad_fk"]), [("g", ("columns",)), ("grad_fk", ("dtype",))],
              extra=dict(grad_fi=False))
        if many_:
            add(entry + "/g/empty stack", fn, D(raw["g"][:0]))
        add(entry + "/g/device", fn, **_wrap(raw))                      # every check passed: the tensors are not on cuda:0 after all
        add(entry + "/grad_fk/device", fn, **dict(_wrap(raw, D0), grad_fk=D(raw["grad_fk"])))
        add(entry + "/solver/not ready", ufn, **_wrap(raw))

    # ---- InterpolationPlan: the constructor's checks that need no handle ----
    xi, x = torch.zeros((10, 2), dtype=f64), torch.zeros((5, 2), dtype=f64)
    I = torch.zeros(5, dtype=torch.int64)
    P = h.InterpolationPlan
    add("InterpolationPlan/mode/value", P, D(xi), 2, D(x), mode="linear")
    add("InterpolationPlan/r/missing", P, D(xi), 2, D(x), mode="continuous")
    add("InterpolationPlan/r/zero", P, D(xi), 2, D(x), mode="continuous", r=0.0)
    add("InterpolationPlan/r/negative", P, D(xi), 2, D(x), mode="continuous", r=-1.5)
    add("InterpolationPlan/I/continuous", P, D(xi), 2, D(x), mode="continuous", r=0.1, I=D(I))
    add("InterpolationPlan/x/numpy", P, D(xi), 2, np.zeros((5, 2)))
    add("InterpolationPlan/x/host", P, D(xi), 2, x)
    add("InterpolationPlan/x/dtype", P, D(xi), 2, D(x.float()))
    add("InterpolationPlan/x/rank", P, D(xi), 2, D(torch.zeros((5, 2, 1), dtype=f64)))
    add("InterpolationPlan/x/coordinates", P, D(xi), 2, D(torch.zeros((5, 4), dtype=f64)))
    add("InterpolationPlan/x/contiguous", P, D(xi), 2, KINDS["contiguous"](x, D))
    add("InterpolationPlan/I/dtype", P, D(xi), 2, D(x), I=D(I.int()))
    add("InterpolationPlan/I/rank", P, D(xi), 2, D(x), I=D(I[:, None]))
    add("InterpolationPlan/I/host", P, D(xi), 2, D(x), I=I)
    add("InterpolationPlan/I/length", P, D(xi), 2, D(x), I=D(I[:4]))
    add("InterpolationPlan/I/contiguous", P, D(xi), 2, D(x), I=KINDS["contiguous"](I, D))
    add("InterpolationPlan/xi/coordinates", P, D(torch.zeros((10, 3), dtype=f64)), 2, D(x))
    add("InterpolationPlan/xi/rank", P, D(torch.zeros((10, 2, 1), dtype=f64)), 2, D(x))
    add("InterpolationPlan/xi/dtype", P, D(xi.float()), 2, D(x))
    add("InterpolationPlan/xi/host", P, xi, 2, D(x))
    add("InterpolationPlan/xi/contiguous", P, KINDS["contiguous"](xi, D), 2, D(x))
    add("InterpolationPlan/xi/empty", P, D(xi[:0]), 2, D(x))
    add("InterpolationPlan/xi/device", P, D(xi), 2, D0(x))
    add("InterpolationPlan/I/device", P, D0(xi), 2, D0(x), I=D(I))
    add("InterpolationPlan/order/dtype", P, D(xi), D(torch.full((10,), 2, dtype=torch.int64)), D(x))
    add("InterpolationPlan/order/rank", P, D(xi), D(torch.full((10, 1), 2, dtype=torch.int32)), D(x))
    add("InterpolationPlan/order/host", P, D(xi), torch.full((10,), 2, dtype=torch.int32), D(x))
    add("InterpolationPlan/order/rows", P, D(xi), D(torch.full((9,), 2, dtype=torch.int32)), D(x))
    add("InterpolationPlan/order/device", P, D0(xi), D(torch.full((10,), 2, dtype=torch.int32)), D0(x))
    add("InterpolationPlan/order/value", P, D(xi), 5, D(x))

    # ---- evaluate, evaluate_adjoint and differentiable_evaluate on a plan without device state ----
    p = _plan()
    fi = torch.zeros((10, 6), dtype=f64)
    add("evaluate/diff/None", p.evaluate, None)
    add("evaluate/diff/36", p.evaluate, list(range(36)))
    add("evaluate/fi/no solver", p.evaluate, 0)
    add("evaluate/fi/dtype", p.evaluate, 0, D(fi.float()))
    add("evaluate/fi/host", p.evaluate, 0, fi)
    add("evaluate/fi/rank", p.evaluate, 0, D(fi[0]))
    add("evaluate/fi/device", p.evaluate, 0, D0(fi))
    add("evaluate/fi/rows", p.evaluate, 0, D(fi[:9]))
    add("evaluate/fi/columns", p.evaluate, 0, D(fi[:, :5]))
    add("evaluate/fi/contiguous", p.evaluate, 0, KINDS["contiguous"](fi, D))
    add("evaluate/fi[stack]/columns", p.evaluate, 0, D(torch.zeros((3, 10, 5), dtype=f64)))
    add("evaluate/out/dtype", p.evaluate, 0, D(fi), out=D(torch.zeros(5)))
    add("evaluate/out/rank", p.evaluate, 0, D(fi), out=D(torch.zeros((1, 5), dtype=f64)))
    add("evaluate/out/shape", p.evaluate, [0, 1], D(fi), out=D(torch.zeros((3, 5), dtype=f64)))
    add("evaluate/out[stack]/shape", p.evaluate, [0, 1], D(torch.zeros((3, 10, 6), dtype=f64)), out=D(torch.zeros((2, 2, 5), dtype=f64)))
    add("evaluate/out/contiguous", p.evaluate, 0, D(fi), out=KINDS["contiguous"](torch.zeros(5, dtype=f64), D))
    g1, g2 = torch.zeros(5, dtype=f64), torch.zeros((2, 5), dtype=f64)
    add("evaluate_adjoint/diff/None", p.evaluate_adjoint, D(g1), None)
    add("evaluate_adjoint/diff/36", p.evaluate_adjoint, D(g1), list(range(36)))
    add("evaluate_adjoint/g/numpy", p.evaluate_adjoint, np.zeros(5))
    add("evaluate_adjoint/g/host", p.evaluate_adjoint, g1)
    add("evaluate_adjoint/g/dtype", p.evaluate_adjoint, D(g1.float()))
    add("evaluate_adjoint/g/rank", p.evaluate_adjoint, D(torch.zeros((1, 2, 5), dtype=f64)))
    add("evaluate_adjoint/g[diffs]/rank", p.evaluate_adjoint, D(g1), [0, 1])
    add("evaluate_adjoint/g/shape", p.evaluate_adjoint, D(torch.zeros(4, dtype=f64)))
    add("evaluate_adjoint/g[diffs]/shape", p.evaluate_adjoint, D(torch.zeros((3, 5), dtype=f64)), [0, 1])
    add("evaluate_adjoint/g/device", p.evaluate_adjoint, D0(g1))
    add("evaluate_adjoint/g/contiguous", p.evaluate_adjoint, KINDS["contiguous"](g2, D), [0, 1])
    add("evaluate_adjoint/ncols/value", p.evaluate_adjoint, D(g1), ncols=5)
    add("evaluate_adjoint/grad_fi/dtype", p.evaluate_adjoint, D(g1), grad_fi=D(fi.float()))
    add("evaluate_adjoint/grad_fi/rank", p.evaluate_adjoint, D(g1), grad_fi=D(fi[None]))
    add("evaluate_adjoint/grad_fi/host", p.evaluate_adjoint, D(g1), grad_fi=fi)
    add("evaluate_adjoint/grad_fi/rows", p.evaluate_adjoint, D(g1), grad_fi=D(fi[:9]))
    add("evaluate_adjoint/grad_fi/columns", p.evaluate_adjoint, D(g1), grad_fi=D(fi), ncols=7)
    add("evaluate_adjoint/grad_fi/contiguous", p.evaluate_adjoint, D(g1), grad_fi=KINDS["contiguous"](fi, D))
    add("evaluate_adjoint/grad_fi/device", p.evaluate_adjoint, D(g1), grad_fi=D0(fi))
    add("evaluate_adjoint/grad_fi[stack]/fields", p.evaluate_adjoint, D(torch.zeros((3, 5), dtype=f64)), grad_fi=D(torch.zeros((2, 10, 6), dtype=f64)))
    closed = _plan()
    closed.close()
    for name, call in (("evaluate", lambda: closed.evaluate(0)), ("evaluate_adjoint", lambda: closed.evaluate_adjoint(D(g1))),
                       ("prepare_adjoint", closed.prepare_adjoint), ("transposed_lists", closed.transposed_lists)):
        add(name + "/plan/closed", call)
    add("lists/plan/nearest", p.lists)
    add("differentiable_evaluate/fi/None", h.differentiable_evaluate, p, None)
    add("differentiable_evaluate/diff/36", h.differentiable_evaluate, p, D(fi), list(range(36)))
    add("differentiable_evaluate/fi/dtype", h.differentiable_evaluate, p, D(fi.float()))
    grad_plan = _plan()
    grad_plan._geometry_requires_grad = True
    add("differentiable_evaluate/plan/requires_grad", h.differentiable_evaluate, grad_plan, D(fi))
    return rows


def outcome(thunk):
    """(exception type name, message) of a row; a row that raises nothing, or reaches the library, has no outcome."""
    from wlsqm import _binding
    real = _binding.lib
    _binding.lib = _no_library
    try:
        thunk()
    except Exception as e:
        return [type(e).__name__, str(e)]
    finally:
        _binding.lib = real
    raise AssertionError("the call raised nothing")


@pytest.fixture(scope="module")
def table():
    pytest.importorskip("torch")
    return json.load(open(TABLE))["rows"]


@pytest.fixture(scope="module")
def rows():
    pytest.importorskip("torch")
    return build_rows()


ENTRY_POINTS = ("fit_many_device", "fit_cloud_device", "fit_many_adjoint_device", "fit_cloud_adjoint_device", "differentiable_fit_many",
                "differentiable_fit_cloud", "differentiable_solve", "differentiable_solve_many", "differentiable_evaluate",
                "solve_device", "solve_many_device", "solve_adjoint_device", "solve_many_adjoint_device", "InterpolationPlan")


def test_the_table_and_the_recording_name_the_same_rows(rows, table):
    assert sorted(rid for rid, _ in rows) == sorted(table)
    assert len(table) >= 400
    for entry in ENTRY_POINTS:
        assert any(rid.split("/")[0].split("[")[0] == entry for rid in table), entry
    for rid, (kind, message) in table.items():
        assert kind in ("ValueError", "RuntimeError") and message, rid
        assert "0x" not in message and "tensor(" not in message, rid


def test_every_row_raises_what_it_raised_before_the_checks_were_shared(rows, table):
    wrong = []
    for rid, thunk in rows:
        try:
            got = outcome(thunk)
        except (AssertionError, _ReachedTheLibrary) as e:
            got = ["no validation error", type(e).__name__]
        if got != table[rid]:
            wrong.append((rid, got, table[rid]))
    for rid, got, want in wrong:
        print("%s\n    now:    %s: %s\n    before: %s: %s" % (rid, got[0], got[1], want[0], want[1]))
    assert not wrong, "%d of %d rows changed, the first: %r" % (len(wrong), len(rows), wrong[0])


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: %s --record   (on the commit the table describes; see the module's docstring)" % sys.argv[0])
    for p in (ROOT, os.path.join(ROOT, "python-wlsqm_amd")):
        sys.path.insert(0, p)
    recorded = {}
    for rid, thunk in build_rows():
        try:
            recorded[rid] = outcome(thunk)
        except BaseException as e:
            sys.exit("%s is not a validation row: %s" % (rid, type(e).__name__))
        if recorded[rid][0] not in ("ValueError", "RuntimeError"):
            sys.exit("%s is not a validation row: %s" % (rid, recorded[rid]))
    with open(TABLE, "w") as f:
        json.dump({"recorded_at": "cec4e7c", "rows": recorded}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d rows" % len(recorded))
