"""StencilOperator.update without a GPU: the two entry points behind it are declared in the header, named by the binding and exported by
the built library; update has the documented signature; and its argument checks, on the OnDevice stub, fail before the library is reached."""
import inspect
import os
import subprocess

import pytest

from _device_helpers import OnDevice

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("wlsqm_hip_stencil_build_device", "wlsqm_hip_sell_permute_device")


def test_header_binding_and_library_name_the_entry_points():
    from wlsqm import _binding
    header = open(os.path.join(ROOT, "include", "wlsqm_hip.h")).read()
    binding = open(os.path.join(ROOT, "python-wlsqm_amd", "wlsqm", "_binding.py")).read()
    for name in SYMBOLS:
        assert "int %s(" % name in header and name in binding, name
    assert "len[j] = clamp(nk[j], 0, max_nk) + (bit F of knowns[j])" in header          # the precondition is stated
    assert os.path.exists(_binding.LIB_PATH), "the library is not built"
    syms = subprocess.run(["nm", "-D", "--defined-only", _binding.LIB_PATH], capture_output=True, text=True).stdout
    for name in SYMBOLS:
        assert " T %s" % name in syms, name
    lib = _binding.lib()
    assert len(lib.wlsqm_hip_stencil_build_device.argtypes) == 25 and len(lib.wlsqm_hip_sell_permute_device.argtypes) == 10


def test_update_has_the_documented_signature():
    import wlsqm.hip as h
    sig = inspect.signature(h.StencilOperator.update)
    assert list(sig.parameters) == ["self", "S", "hoods", "rows", "check", "stream"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert d["hoods"] is None and d["rows"] is None and d["check"] is True and d["stream"] is None
    assert d["S"] is inspect.Parameter.empty
    assert "invalidates" in h.differentiable_stencil_apply.__doc__


class _ReachedTheLibrary(BaseException):
    pass


def _raises(kind, message, fn, *args, **kw):
    from wlsqm import _binding

    def no_library():
        raise _ReachedTheLibrary()

    real = _binding.lib
    _binding.lib = no_library
    try:
        with pytest.raises(kind, match=message):
            fn(*args, **kw)
    finally:
        _binding.lib = real


def test_argument_checks_need_no_device():
    import wlsqm.hip as h
    D = OnDevice
    f64 = torch.float64
    n, K, npoints, no, nop = 4, 7, 10, 6, 2
    S = torch.rand((npoints, 2), dtype=f64)
    hoods = torch.ones((n, K), dtype=torch.int32)
    geo = (D(hoods), D(torch.full((n,), K, dtype=torch.int32)), D(torch.zeros((n,), dtype=torch.int64)),
           D(torch.full((n,), 2, dtype=torch.int32)), None)

    def shell(rows):
        op = h.StencilOperator.__new__(h.StencilOperator)
        op._m, op._t, op._tval, op._tpair = dict(total=0), None, None, None
        op.nop, op.ncases, op.npoints, op.K, op.no, op._device = nop, n, npoints, K, no, torch.device("cpu")
        op.dimension, op.order = 2, 2
        op._val = torch.zeros((nop, 0), dtype=f64)
        op.known_coef, op.has_known_derivatives, op._structural = torch.zeros((nop, n, no), dtype=f64), False, False
        op._geo, op._rows = geo, D(rows)
        return op

    op = shell(torch.ones((nop, no), dtype=f64))
    _raises(ValueError, "expected 'float64'.*argument S", op.update, D(S.float()))
    _raises(ValueError, "must be a device", op.update, S)
    _raises(ValueError, "must be contiguous", op.update, D(S.t().contiguous().t()))
    _raises(ValueError, "wrong number of dimensions.*argument S", op.update, D(S[:, 0].contiguous()))
    _raises(ValueError, "S has fewer points than the operator's npoints = 10", op.update, D(S[:9]))
    _raises(ValueError, "expected 'int32'.*argument hoods", op.update, D(S), hoods=D(hoods.long()))
    _raises(ValueError, "another shape needs a new operator", op.update, D(S), hoods=D(torch.ones((n, K + 1), dtype=torch.int32)))
    _raises(ValueError, "another shape needs a new operator", op.update, D(S), hoods=D(torch.ones((n + 1, K), dtype=torch.int32)))
    _raises(ValueError, "contiguous last axis", op.update, D(S), hoods=D(torch.ones((n, 2 * K), dtype=torch.int32)[:, ::2]))
    _raises(ValueError, "rows must keep the operator's form, \\(nop, no\\) with nop = 2", op.update, D(S), rows=D(torch.ones((3, no), dtype=f64)))
    _raises(ValueError, "rows must keep the operator's form", op.update, D(S), rows=D(torch.ones((nop, n, no), dtype=f64)))
    _raises(ValueError, "expected 'float64'.*argument rows", op.update, D(S), rows=D(torch.ones((nop, no))))
    _raises(ValueError, "rows has 5 columns", op.update, D(S), rows=D(torch.ones((nop, 5), dtype=f64)))
    _raises(ValueError, "not contiguous in the same dimension. \\(argument rows\\)", op.update, D(S), rows=D(torch.ones((nop, 2 * no), dtype=f64)[:, ::2]))
    per = shell(torch.ones((nop, n, no), dtype=f64))
    _raises(ValueError, "rows must keep the operator's form, \\(nop, ncases, no\\)", per.update, D(S), rows=D(torch.ones((nop, no), dtype=f64)))
    _raises(ValueError, "rows has 3 rows, fewer than the 4 cases", per.update, D(S), rows=D(torch.ones((nop, 3, no), dtype=f64)))
    # no fit to redo; closed
    co = h.StencilOperator.__new__(h.StencilOperator)
    co._m, co._geo = dict(total=0), None
    _raises(RuntimeError, "made from coefficients: there is no fit to redo", co.update, D(S))
    op.close()
    _raises(RuntimeError, "the stencil operator has been closed", op.update, D(S))
