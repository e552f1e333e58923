"""The stacked right-hand sides without a GPU (wlsqm.hip.StencilSolver(nfields=...), csrc/krylov.hip's krylov_*_many, DESIGN.md section
20): the entry points in header, binding and library; the size of the workspace as a function of nfields (monotone, a step exactly at
each pitch, never below the single-field one); the argument checks on the OnDevice stub, which run before the library is reached."""
import os

import numpy as np
import pytest

from _device_helpers import OnDevice
from test_krylov_host import _operator, _raises

torch = pytest.importorskip("torch")

NAMES = ["wlsqm_hip_krylov_many_workspace_bytes", "wlsqm_hip_krylov_many_start_device", "wlsqm_hip_krylov_many_bicgstab_device",
         "wlsqm_hip_krylov_many_product_device"]


def test_header_binding_and_library_name_the_entry_points():
    import subprocess
    from wlsqm import _binding
    import wlsqm.hip as h
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "wlsqm_hip.h")).read()
    binding = open(os.path.join(root, "python-wlsqm_amd", "wlsqm", "_binding.py")).read()
    for name in NAMES:
        assert " %s(" % name in header
    assert "wlsqm_hip_krylov_many_workspace_bytes" in binding and 'wlsqm_hip_krylov_many_%s_device' in binding
    for kernel in ("krylov-spmv-many", "krylov-update-many", "krylov-update-block-many", "krylov-reduce-many"):
        assert '"%s"' % kernel in header
    syms = subprocess.run(["nm", "-D", "--defined-only", _binding.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        assert " T %s" % name in syms
        assert getattr(_binding.lib(), name).argtypes is not None
    assert "differentiable_stencil_solve_many" in h.__all__
    for method in ("solve_many", "enqueue_many", "info_many", "product_many"):
        assert callable(getattr(h.StencilSolver, method))


@pytest.mark.parametrize("nrows", (1, 64, 130, 257, 65537, 10 ** 6))
def test_workspace_bytes(nrows):
    from wlsqm import _binding
    L = _binding.lib()
    size = [L.wlsqm_hip_krylov_many_workspace_bytes(nrows, f) for f in range(1, 9)]
    single = L.wlsqm_hip_krylov_workspace_bytes(nrows)
    assert all(a <= b for a, b in zip(size, size[1:]))                   # monotone in nfields
    steps = [f + 1 for f in range(1, 8) if size[f] != size[f - 1]]       # the nfields at which the size changes
    assert steps == [3, 5], steps                                        # exactly where the pitch goes 2 -> 4 -> 8
    assert min(size) >= single
    nwg = (nrows + 255) // 256
    for nfields, pitch in ((1, 2), (2, 2), (3, 4), (4, 4), (5, 8), (8, 8)):
        # 9 blocks of 128 bytes, the partials (2 sums x pitch fields x workgroups, rounded to 8 doubles), 8 vectors at the pitch, dinv
        assert size[nfields - 1] == 8 * (144 + (2 * pitch * nwg + 7) // 8 * 8 + 8 * pitch * nrows + nrows)
    for bad in ((-1, 2), (nrows, 0), (nrows, 9), (nrows, -1)):
        assert L.wlsqm_hip_krylov_many_workspace_bytes(*bad) == -1


def test_argument_checks_need_no_device():
    import wlsqm.hip as h
    from wlsqm import _binding
    D = OnDevice
    f64 = torch.float64
    n = 130
    op = _operator(n)
    for bad in (0, 9, -1, True, 2.0, None):
        _raises("nfields must be an int, 1 .. 8", h.StencilSolver, op, nfields=bad)
    L = _binding.lib()
    # nfields = 1 allocates what a solver without the argument does; above it, what the library says
    assert h.StencilSolver(op, nfields=1).memory_used() == h.StencilSolver(op).memory_used() == L.wlsqm_hip_krylov_workspace_bytes(n)
    diag = torch.full((n,), 2.0, dtype=f64)
    solver = h.StencilSolver(op, o=1, diag=D(diag), scale=-0.75, nfields=3)
    assert solver.nfields == 3 and solver.memory_used() == L.wlsqm_hip_krylov_many_workspace_bytes(n, 3)
    blocked = h.StencilSolver(op, preconditioner=h.BlockJacobi(16), nfields=8)
    assert blocked.memory_used() == L.wlsqm_hip_krylov_many_workspace_bytes(n, 8) + L.wlsqm_hip_krylov_block_bytes(n, 16)
    b, x = torch.zeros((3, n), dtype=f64), torch.zeros((3, n), dtype=f64)
    both = torch.zeros((6, n), dtype=f64)
    for call in (solver.solve_many, lambda b_, x_, **kw: solver.enqueue_many(b_, x_, 5, **kw)):
        _raises("argument b must be a device", call, b, D(x))
        _raises("argument x must be a device", call, D(b), np.zeros((3, n)))
        _raises("expected 'float64'.*argument b", call, D(b.float()), D(x))
        _raises("wrong number of dimensions.*argument x", call, D(b), D(x[0]))
        _raises("b must be a float64 device tensor of shape \\(3, 130\\), one row per field.*got shape \\(2, 130\\)", call, D(b[:2]), D(x))
        _raises("x must be a float64 device tensor of shape \\(3, 130\\).*got shape \\(3, 129\\)", call, D(b), D(x[:, :-1]))
        _raises("b overlaps x", call, D(both[:3]), D(both[2:5]))
        _raises("b overlaps x", call, D(both[::2]), D(both[1::2]))        # extents, as everywhere: interleaved rows count as overlapping
        _raises("b overlaps diag", call, D(diag[None].expand(3, n)), D(x))
        _raises("b overlaps workspace", call, D(solver._ws[:3 * n].view(3, n)), D(x))
        _raises("the elements of x must be distinct in memory; got strides \\(0, 1\\)", call, D(b), D(x[:1].expand(3, n)))
        _raises("the elements of x must be distinct in memory", call, D(b), D(torch.zeros(n + 2, dtype=f64).as_strided((3, n), (1, 1))))
        _raises("rtol and atol must be finite and >= 0", call, D(b), D(x), rtol=-1.0)
    _raises("check_every must be >= 1", solver.solve_many, D(b), D(x), check_every=0)
    _raises("the number of iterations must be", solver.solve_many, D(b), D(x), maxiter=-1)
    _raises("the number of iterations must be", solver.enqueue_many, D(b), D(x), 2 ** 31)
    _raises("v overlaps out", solver.product_many, D(both[:3]), out=D(both[2:5]))
    _raises("w must be a float64 device tensor of shape \\(3, 130\\)", solver.product_many, D(b), D(b[:2]), out=D(x))
    _raises("the elements of out must be distinct in memory", solver.product_many, D(b), out=D(x[:1].expand(3, n)))
    _raises("solver must be a StencilSolver", h.differentiable_stencil_solve_many, object(), D(b))
    _raises("x0 must be a float64 device tensor of shape \\(3, 130\\)", h.differentiable_stencil_solve_many, solver, D(b), x0=D(x[:2]))
    _raises("check_every must be >= 1", h.differentiable_stencil_solve_many, solver, D(b), check_every=0)
    # any strides pass the checks; b may repeat one right-hand side
    point_major = torch.zeros((n, 3), dtype=f64)
    for ok_b, ok_x in ((D(b), D(point_major.T)), (D(both[::2]), D(x)), (D(b[:1].expand(3, n)), D(x))):
        solver._fields(written=("x",), b=ok_b, x=ok_x)
    # a solver of one field takes (1, npoints)
    one = h.StencilSolver(op)
    _raises("b must be a float64 device tensor of shape \\(1, 130\\).*got shape \\(3, 130\\)", one.solve_many, D(b), D(x))
    solver.close()
    for call in (lambda: solver.solve_many(D(b), D(x)), lambda: solver.enqueue_many(D(b), D(x), 3), solver.info_many,
                 lambda: solver.product_many(D(b))):
        _raises("the stencil solver has been closed", call)
