"""Device-resident entry points of the HIP backend (extension to the reference surface).

The reference API (wlsqm.fitter.simple / expert) takes host arrays, so every call pays PCIe for
8*nk*(dim+1) bytes per case.  These functions take arrays that already live in HBM — torch CUDA
tensors, or anything exposing ``data_ptr()``/``stride()``/``shape``/``dtype`` the same way — and
enqueue the same kernels on the caller's HIP stream with no host synchronisation.  torch is used
only as the owner of device memory and streams.
"""
import ctypes as C

from . import _binding as B

import collections
import contextlib

__all__ = ["fit_many_device", "time_fit_device", "fit_cloud_device", "time_fit_cloud_device", "device_count", "knn", "ball", "nearest",
           "fit_many_adjoint_device", "fit_cloud_adjoint_device", "fit_many_geometry_adjoint_device",
           "fit_cloud_geometry_adjoint_device", "differentiable_fit_many", "differentiable_fit_cloud",
           "differentiable_solve", "differentiable_solve_many",
           "InterpolationPlan", "differentiable_evaluate",
           "StencilOperator", "stencil_rows", "differentiable_stencil_apply", "StencilSolver", "StencilSystemSolver", "SolveInfo",
           "SolveGradients", "BlockJacobi", "ApproximateInverse", "OverlappingBlocks", "PointBlockJacobi", "differentiable_stencil_solve", "differentiable_stencil_solve_many",
           "SystemGradients", "differentiable_stencil_system_solve", "SpatialOrder", "last_kernel", "set_strict", "get_strict", "strict", "accurate", "contracted", "strict_intermediates",
           "getrf_batched", "getrs_batched", "gesv_batched", "sytrf_batched", "sytrs_batched", "sysv_batched", "symmetrize_batched"]


def _mode_code(mode):
    """False / 0 -> 0 (fast), True / 1 / "strict" -> 1, 2 / "accurate" -> 2, 3 / "contracted" -> 3."""
    if isinstance(mode, str):
        m = mode.lower()
        if m in ("contracted", "3"):
            return 3
        if m in ("accurate", "2"):
            return 2
        if m in ("strict", "1", "true"):
            return 1
        if m in ("fast", "0", "false", ""):
            return 0
        raise ValueError("numerics mode must be 'fast', 'strict', 'accurate' or 'contracted', got %r" % (mode,))
    if mode is True:
        return 1
    return int(mode) if int(mode) in (2, 3) else (1 if mode else 0)


def set_strict(on):
    """Numerics mode of the calling thread (wlsqm_hip_set_strict): False = the fast kernels (default, or WLSQM_HIP_STRICT in
    the environment), True / "strict" = reference-order arithmetic (csrc/fit_strict.hip: the reference's operations one for one,
    IEEE divide and sqrt, no contraction), 2 / "accurate" = the same arithmetic with the normal
    matrix assembled from its upper triangle (csrc/fit_accurate.hip: as close to the reference as the strict mode — 1e-10 on every
    column of BASELINE configs[1] / configs[4] — at a fraction of its time; cases it does not cover run the strict kernels),
    3 / "contracted" = the accurate mode with its neighbour sums, LU update and substitutions fused (a <- fma(b, c, a); the same
    kernels and coverage; still within 1e-10 on every column of those configs, with a thinner margin: 9.0e-11 on the 16M-point
    configs[4] sample).
    Returns the previous mode: False, True, 2 or 3."""
    prev = B.lib().wlsqm_hip_set_strict(_mode_code(on))
    return prev if prev in (2, 3) else bool(prev)


def get_strict():
    """False (fast), True (strict), 2 (accurate) or 3 (contracted)."""
    v = B.lib().wlsqm_hip_get_strict()
    return v if v in (2, 3) else bool(v)


@contextlib.contextmanager
def strict(on=True):
    """``with wlsqm.hip.strict(): ...`` — reference-order numerics inside the block (None: leave the mode alone;
    ``strict("accurate")`` / ``strict(2)``: the accurate mode; ``strict("contracted")`` / ``strict(3)``: the contracted mode)."""
    if on is None:
        yield
        return
    prev = set_strict(on)
    try:
        yield
    finally:
        set_strict(prev)


def accurate():
    """``with wlsqm.hip.accurate(): ...`` — the accurate numerics mode inside the block."""
    return strict(2)


def contracted():
    """``with wlsqm.hip.contracted(): ...`` — the contracted numerics mode (the accurate mode with fused sums) inside the block."""
    return strict(3)


def device_count():
    return B.lib().wlsqm_hip_device_count()


def last_kernel():
    """Diagnostics: name of the kernel family the last fit launch of this thread dispatched to (wlsqm_hip_last_kernel)."""
    return B.lib().wlsqm_hip_last_kernel().decode()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _check(t, name, dtype_name, ndim):
    if str(t.dtype).split(".")[-1] != dtype_name:
        raise ValueError("Buffer dtype mismatch, expected '%s' but got '%s' (argument %s)" % (dtype_name, t.dtype, name))
    if t.dim() != ndim:
        raise ValueError("Buffer has wrong number of dimensions (expected %d, got %d) (argument %s)" % (ndim, t.dim(), name))
    if not t.is_cuda:
        raise ValueError("argument %s must be a device (HIP) tensor" % name)


_NDOF = {1: (1, 2, 3, 4, 5), 2: (1, 3, 6, 10, 15), 3: (1, 4, 10, 20, 35)}


def _ndofs(dimension, order):
    if dimension not in _NDOF:
        raise ValueError("Dimension must be 1, 2 or 3")
    if not 0 <= int(order) <= 4:
        raise ValueError("order must be 0, 1, 2, 3 or 4")
    return _NDOF[dimension][int(order)]


_FEW_ROWS = "%s has %d rows, fewer than the %d cases of the batch"


def _rows(n, **arrays):
    """Every per-case array must cover the n cases of the launch (simple.py's _run_many makes the same checks on the host)."""
    for name, t in arrays.items():
        if t.shape[0] < n:
            raise ValueError(_FEW_ROWS % (name, t.shape[0], n))


def _double_rows(t, name, nrows, ncols, of=None, says=None, lead=0):
    """fi, g, grad_fi, slots: a float64 device tensor (>= nrows, >= ncols) with a contiguous last axis.  `of`: the (dimension, order)
    that ncols is the number of DOFs of, for the callers whose message names them; `says` is a caller's own sentence for a wrong
    layout or extent, raised in place of the three below; `lead`: the number of axes in front of the rows (a stack of such tensors)."""
    _check(t, name, "float64", 2 + lead)
    if says is not None:
        if t.shape[lead] < nrows or t.shape[lead + 1] < ncols or t.stride(lead + 1) != 1:
            raise ValueError(says)
        return
    if t.stride(lead + 1) != 1:
        raise ValueError("Buffer and memoryview are not contiguous in the same dimension. (argument %s)" % name)
    if t.shape[lead] < nrows:
        raise ValueError(_FEW_ROWS % (name, t.shape[lead], nrows))
    if t.shape[lead + 1] < ncols:
        raise ValueError("%s has %d columns, need at least number_of_dofs%s = %d" % (name, t.shape[lead + 1], "(%d, %d)" % of if of else "", ncols))


def _dense_geometry(dimension, xk, nk, xi, knowns, weighting_method):
    """The geometry of a dense batch, checked and put into a B.Batch (the forward adds fk, fi and sens, the adjoint g and its outputs):
    xk (n, K, dim) [1D: (n, K)], nk (n,) int32, xi (n, dim) [1D: (n,)], knowns (n,) int64, weighting_method (n,) int32."""
    ncases = nk.shape[0]
    _check(nk, "nk", "int32", 1); _check(knowns, "knowns", "int64", 1); _check(weighting_method, "weighting_method", "int32", 1)
    if dimension == 1:
        _check(xk, "xk", "float64", 2); _check(xi, "xi", "float64", 1)
    else:
        _check(xk, "xk", "float64", 3); _check(xi, "xi", "float64", 2)
        if xk.stride(2) != 1 or xi.stride(1) != 1:
            raise ValueError("Buffer and memoryview are not contiguous in the same dimension.")
        if xk.shape[2] < dimension or xi.shape[1] < dimension:
            raise ValueError("xk / xi must have %d coordinates on the last axis" % dimension)
    _rows(ncases, xk=xk, xi=xi, knowns=knowns, weighting_method=weighting_method)
    b = B.Batch()
    b.dimension, b.ncases = dimension, ncases
    b.xk, b.xk_stride_case, b.xk_stride_k = xk.data_ptr(), xk.stride(0), xk.stride(1)
    b.nk, b.nk_stride = nk.data_ptr(), nk.stride(0)
    b.xi, b.xi_stride_case = xi.data_ptr(), xi.stride(0)
    b.knowns, b.knowns_stride = knowns.data_ptr(), knowns.stride(0)
    b.weighting_method, b.wm_stride = weighting_method.data_ptr(), weighting_method.stride(0)
    return b


def _batch(dimension, order, xk, fk, nk, xi, fi, knowns, weighting_method, sens, iterative, max_iter, order_dummy):
    no = _ndofs(dimension, order)
    b = _dense_geometry(dimension, xk, nk, xi, knowns, weighting_method)
    ncases = b.ncases
    # extents: the kernels write `no` doubles per fi row at the row pitch and read K neighbour slots per xk / fk row
    _check(fk, "fk", "float64", 2)
    if fk.shape[0] < ncases:
        raise ValueError(_FEW_ROWS % ("fk", fk.shape[0], ncases))
    K = int(fk.shape[1])
    if xk.shape[1] < K:
        raise ValueError("xk has %d neighbour slots per case, fk has %d" % (xk.shape[1], K))
    _double_rows(fi, "fi", ncases, no, (dimension, order))
    if sens is not None:
        _check(sens, "sens", "float64", 3)
        if sens.stride(2) != 1:
            raise ValueError("Buffer and memoryview are not contiguous in the same dimension. (argument sens)")
        if sens.shape[0] < ncases or sens.shape[1] < K or sens.shape[2] < no:
            raise ValueError("sens must be at least (ncases, %d, %d); got %s" % (K, no, tuple(sens.shape)))
        b.do_sens = 1
        b.sens, b.sens_stride_case, b.sens_stride_k = sens.data_ptr(), sens.stride(0), sens.stride(1)
    b.fk, b.fk_stride_case, b.fk_stride_k = fk.data_ptr(), fk.stride(0), fk.stride(1)
    b.fi, b.fi_stride_case = fi.data_ptr(), fi.stride(0)
    # the per-case order array is not read on this path (order_uniform is); point it somewhere valid
    b.order, b.order_stride = order_dummy.data_ptr(), 0
    b.iterative, b.max_iter, b.max_nk = (1 if iterative else 0), int(max_iter), K
    return b


def _case_index(case_index):
    """(pointer, count) of the cases a launch is restricted to (an int64 device tensor), (None, 0) without one."""
    if case_index is None:
        return None, 0
    _check(case_index, "case_index", "int64", 1)
    return C.c_void_p(case_index.data_ptr()), int(case_index.shape[0])


def _strict_ctx(flag):
    # the entry points below take a `strict=` parameter, which hides the context manager of that name inside them
    return strict(flag)


def _stream_ptr(where, stream):
    """The HIP stream of a launch as a c_void_p: `stream`, or (None) torch's current stream on the device of `where`, a tensor, a
    torch device or a device number (None: torch's current device)."""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream(getattr(where, "device", where)).cuda_stream
    return C.c_void_p(int(stream) if stream else 0)


def _stream_and_device(t, stream):
    dev = t.device.index
    if dev is None:
        import torch
        dev = torch.cuda.current_device()
    return _stream_ptr(dev, stream), dev


class row_hint:
    """with wlsqm.hip.row_hint("ragged"): ... — what the calling thread knows about the neighbour counts of the dense device-resident batches
    it hands over (wlsqm_hip_set_row_hint): "full" (default: every case fills its row), "ragged" (e.g. ball-query rows: the staged kernels'
    waves move only the chunks their own cases need) or None / "unknown" (the kernels find out: one idle launch for full rows).  A hint: the
    results are the same bits either way."""
    _CODE = {"full": 1, True: 2, "ragged": 2, None: 0, "unknown": 0, False: 1}

    def __init__(self, what="full", sorted=True):
        # sorted: the neighbours of every row come sorted by distance (a k-nearest-neighbour search's rows: the default) or not (a ball
        # query's: sorted=False) — wlsqm_hip_set_order_hint: picks the form of the staged kernels of the small dense systems
        self.code = self._CODE[what]
        self.sorted = 1 if sorted else 0

    def __enter__(self):
        L = B.lib()
        self.prev = L.wlsqm_hip_set_row_hint(self.code) if hasattr(L, "wlsqm_hip_set_row_hint") else 1
        self.prev_sorted = L.wlsqm_hip_set_order_hint(self.sorted) if hasattr(L, "wlsqm_hip_set_order_hint") else 1
        return self

    def __exit__(self, *exc):
        L = B.lib()
        if hasattr(L, "wlsqm_hip_set_row_hint"):
            L.wlsqm_hip_set_row_hint(self.prev)
        if hasattr(L, "wlsqm_hip_set_order_hint"):
            L.wlsqm_hip_set_order_hint(self.prev_sorted)
        return False


def fit_many_device(dimension, order, xk, fk, nk, xi, fi, knowns, weighting_method, sens=None, iterative=False,
                    max_iter=10, case_index=None, stream=None, want_iterations=False, strict=None, max_order=4):
    """fit_{1,2,3}D[_iterative]_many on device-resident tensors.  `order`: an int (all cases of that polynomial order: the fast
    path) or an int32 device tensor of per-case orders (fi / sens must then be wide enough for `max_order`, default 4: the
    reference's "(ncases, >= max no)" rule with the maximum taken from the caller instead of a host scan of the tensor).
    strict=True / False selects reference-order / fast numerics for this call (None: the thread's mode, see set_strict).

    xk (n, K, dim) [1D: (n, K)], fk (n, K), nk (n,) int32, xi (n, dim) [1D: (n,)], fi (n, >=no) in/out,
    knowns (n,) int64, weighting_method (n,) int32, sens (n, K, >=no) or None.  `case_index` (int64 device
    tensor) restricts the launch to those cases (used to bucket heterogeneous orders).  Asynchronous on
    `stream` (default: torch's current stream) unless want_iterations=True.  The caller guarantees that
    fk/xk do not alias fi (outputs are written in place)."""
    if hasattr(order, "data_ptr"):
        # per-case orders (int32 device tensor, as the reference's `order` array): bucketed on the device, no host synchronisation
        _check(order, "order", "int32", 1)
        if case_index is not None:
            raise ValueError("case_index and a per-case order tensor exclude each other")
        _rows(nk.shape[0], order=order)
        # extents are checked for `max_order` (default 4): the caller's promise that no case asks for more
        b = _batch(dimension, int(max_order), xk, fk, nk, xi, fi, knowns, weighting_method, sens, iterative, max_iter, nk)
        s, dev = _stream_and_device(fi, stream)
        its = C.c_int32(0)
        with _strict_ctx(strict):
            B.check(B.lib().wlsqm_hip_fit_many_device_orders(C.byref(b), dev, s, C.c_void_p(order.data_ptr()), order.stride(0),
                                                             int(max_order), C.byref(its) if want_iterations else None))
        return int(its.value)
    b = _batch(dimension, order, xk, fk, nk, xi, fi, knowns, weighting_method, sens, iterative, max_iter, nk)
    s, dev = _stream_and_device(fi, stream)
    its = C.c_int32(0)
    ci, nsel = _case_index(case_index)
    with _strict_ctx(strict):
        B.check(B.lib().wlsqm_hip_fit_many_device(C.byref(b), dev, s, int(order), ci, nsel,
                                                  C.byref(its) if want_iterations else None))
    return int(its.value)


def strict_intermediates(dimension, order, xk, fk, nk, xi, fi, knowns, weighting_method, stream=None):
    """Test hook (wlsqm_hip_strict_intermediates_device): the reference-order fit of a uniform-order batch, which also returns
    the reference's intermediates as device tensors: dict(w (n, K), A (n, no*no), LU (n, no*no), row_scale (n, no),
    col_scale (n, no), ipiv (n, no) int32).  A / LU hold the nr x nr Fortran-order block of each case at the front of its row."""
    import torch
    b = _batch(dimension, order, xk, fk, nk, xi, fi, knowns, weighting_method, None, False, 0, nk)
    s, dev = _stream_and_device(fi, stream)
    n, K, no = int(nk.shape[0]), int(fk.shape[1]), _ndofs(dimension, order)
    z = lambda *shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=fi.device)
    out = dict(w=z(n, K), A=z(n, no * no), LU=z(n, no * no), row_scale=z(n, no), col_scale=z(n, no), ipiv=z(n, no, dt=torch.int32))
    B.check(B.lib().wlsqm_hip_strict_intermediates_device(C.byref(b), dev, s, int(order), _ptr(out["w"]), K, _ptr(out["A"]),
                                                          _ptr(out["LU"]), no * no, _ptr(out["row_scale"]), _ptr(out["col_scale"]),
                                                          _ptr(out["ipiv"]), no))
    return out


def time_fit_device(dimension, order, xk, fk, nk, xi, fi, knowns, weighting_method, reps=10, stream=None):
    """Mean duration in milliseconds of one fit launch (HIP events on `stream`, `reps` back-to-back launches)."""
    b = _batch(dimension, order, xk, fk, nk, xi, fi, knowns, weighting_method, None, False, 0, nk)
    s, dev = _stream_and_device(fi, stream)
    ms = C.c_float(0.0)
    B.check(B.lib().wlsqm_hip_time_fit_device(C.byref(b), dev, s, int(order), int(reps), C.byref(ms)))
    return float(ms.value)


def _cloud_geometry(dimension, S, hoods, nk, knowns, weighting_method, point_index, layout):
    """The geometry of an index-based batch, checked (the forward adds F, fi and sens, the adjoint g and its outputs): S (npoints, dim)
    [1D: (npoints,)] contiguous, hoods (ncases, K) int32, nk / knowns / weighting_method per case with unit stride, point_index
    (ncases,) int32 or None.  `layout` is the caller's sentence about contiguity, which also names its own arrays.  Returns
    (ncases, K)."""
    _check(hoods, "hoods", "int32", 2)
    _check(S, "S", "float64", 1 if dimension == 1 else 2)
    _check(nk, "nk", "int32", 1); _check(knowns, "knowns", "int64", 1); _check(weighting_method, "weighting_method", "int32", 1)
    if not S.is_contiguous() or hoods.stride(1) != 1:
        raise ValueError(layout)
    for t in (nk, knowns, weighting_method):
        if t.stride(0) != 1:
            raise ValueError("nk, knowns, weighting_method must have unit stride")
    ncases, K = int(hoods.shape[0]), int(hoods.shape[1])
    _rows(ncases, nk=nk, knowns=knowns, weighting_method=weighting_method)
    if point_index is not None:
        _check(point_index, "point_index", "int32", 1)
        _rows(ncases, point_index=point_index)
    elif S.shape[0] < ncases:
        raise ValueError("S has %d points but there are %d cases (xi of case j is S[j] without point_index)" % (S.shape[0], ncases))
    if dimension > 1 and S.shape[1] != dimension:
        raise ValueError("S must be (npoints, %d)" % dimension)
    return ncases, K


def _cloud_args(dimension, order, S, F, hoods, fi, nk, knowns, weighting_method, point_index):
    no = _ndofs(dimension, order)
    layout = "S, F must be contiguous; hoods and fi must have a contiguous last axis"
    _check(F, "F", "float64", 1); _check(fi, "fi", "float64", 2)
    if not F.is_contiguous() or fi.stride(1) != 1:
        raise ValueError(layout)
    ncases, K = _cloud_geometry(dimension, S, hoods, nk, knowns, weighting_method, point_index, layout)
    if F.shape[0] < S.shape[0]:
        raise ValueError("F has fewer entries than S has points")
    _double_rows(fi, "fi", ncases, no, (dimension, order))
    return [int(dimension), int(order), ncases, K, _ptr(S), _ptr(F), _ptr(hoods), int(hoods.stride(0)), _ptr(point_index),
            _ptr(nk), _ptr(knowns), _ptr(weighting_method), _ptr(fi), int(fi.stride(0))]


def fit_cloud_device(dimension, order, S, F, hoods, fi, nk, knowns, weighting_method, point_index=None, sens=None,
                     iterative=False, max_iter=10, stream=None, want_iterations=False, strict=None):
    """Index-based fit (extension): the kernels gather xk = S[hoods], fk = F[hoods] themselves.

    S (npoints, dim) [1D: (npoints,)] and F (npoints,) are the device-resident point tables, hoods (ncases, K)
    int32 the neighbour lists, xi of case j is S[point_index[j]] (default: S[j]); nk/knowns/weighting_method
    per case; fi (ncases, >= no) in/out.  Only the slots k < nk[j] of a hoods row are dereferenced (the padding of a ragged
    row may hold anything, e.g. -1 or npoints as scipy pads); those must be valid point numbers.  Asynchronous on `stream`
    unless want_iterations=True (returns the maximum refinement count; otherwise 0).  4 nk bytes of indices per fit instead of 8 nk (dim+1) bytes of gathered
    coordinates; order the points along a space-filling curve (wlsqm.hip.SpatialOrder) so that the gathers hit L2."""
    a = _cloud_args(dimension, order, S, F, hoods, fi, nk, knowns, weighting_method, point_index)
    s, dev = _stream_and_device(fi, stream)
    ss = (int(sens.stride(0)), int(sens.stride(1))) if sens is not None else (0, 0)
    if sens is not None:
        _check(sens, "sens", "float64", 3)
        if sens.stride(2) != 1 or sens.shape[0] < hoods.shape[0] or sens.shape[1] < hoods.shape[1] \
                or sens.shape[2] < _ndofs(dimension, order):
            raise ValueError("sens must be at least (ncases, max_nk, no) with a contiguous last axis; got %s" % (tuple(sens.shape),))
    its = C.c_int32(0)
    with _strict_ctx(strict):
        B.check(B.lib().wlsqm_hip_fit_cloud_device(*a, _ptr(sens), ss[0], ss[1], 1 if sens is not None else 0,
                                                   1 if iterative else 0, int(max_iter), dev, s,
                                                   C.byref(its) if want_iterations else None))
    return int(its.value)


def time_fit_cloud_device(dimension, order, S, F, hoods, fi, nk, knowns, weighting_method, point_index=None, reps=10,
                          stream=None):
    """Mean duration in milliseconds of one index-based fit launch (HIP events on `stream`)."""
    a = _cloud_args(dimension, order, S, F, hoods, fi, nk, knowns, weighting_method, point_index)
    s, dev = _stream_and_device(fi, stream)
    ms = C.c_float(0.0)
    B.check(B.lib().wlsqm_hip_time_fit_cloud_device(*a, dev, s, int(reps), C.byref(ms)))
    return float(ms.value)


# ---- the adjoint of the fit: gradients through device-resident fits (csrc/fit_adjoint.hip) ----

def _adjoint_order(dimension, order):
    if hasattr(order, "data_ptr"):
        raise ValueError("the adjoint takes an integer order (one polynomial order for the whole batch)")
    no = _ndofs(dimension, order)
    if dimension == 3 and int(order) >= 3:
        raise ValueError("fit_adjoint: unsupported (dimension, order)")
    return no


def fit_many_adjoint_device(dimension, order, xk, nk, xi, knowns, weighting_method, g, grad_fk=None, grad_fi=None, case_index=None,
                            stream=None):
    """The vector-Jacobian product of fit_many_device (basic fit, integer `order`): given g (n, >= no) = dL/dfi_out, returns
    (grad_fk, grad_fi) = (dL/dfk (n, K), dL/dfi_in (n, no)).  The fit is linear in fk and in the known entries of fi, so neither
    enters: the geometry arguments are those of fit_many_device (xk (n, K, dim) [1D: (n, K)], nk, xi, knowns, weighting_method).

    grad_fk[j, k] is exactly 0 for nk[j] <= k; grad_fi[j, a] is g[j, a] minus the fit's dependence on the value for a known DOF, g[j, a]
    for a DOF dropped by stray high mask bits, 0 for an unknown (its incoming value is never read); a case with every DOF known has
    grad_fk = 0 and grad_fi = g.  The outputs are allocated when not given (with `case_index`: zero-filled, the kernel writes the
    selected rows only); grad_fi=False: not wanted (returned as None); grad_fi may be g itself.  One kernel launch on `stream`
    (default: torch's current stream), no allocation when both outputs are given, no synchronisation: it can be captured.
    The arithmetic is always the fast kernels' (FMA, LDL^T), whatever numerics mode the forward fit ran in: the modes round the
    same linear map differently.  3D orders 3 and 4 are not covered (ValueError)."""
    import torch
    no = _adjoint_order(dimension, order)
    b = _dense_geometry(dimension, xk, nk, xi, knowns, weighting_method)
    ncases, K = b.ncases, int(xk.shape[1])
    b.max_nk = K
    _double_rows(g, "g", ncases, no)
    new = torch.zeros if case_index is not None else torch.empty
    if grad_fk is None:
        grad_fk = new((ncases, K), dtype=torch.float64, device=g.device)
    _check(grad_fk, "grad_fk", "float64", 2)
    _rows(ncases, grad_fk=grad_fk)
    if grad_fk.shape[1] < K:
        raise ValueError("grad_fk has %d neighbour slots per case, xk has %d" % (grad_fk.shape[1], K))
    if grad_fi is None:
        grad_fi = new((ncases, no), dtype=torch.float64, device=g.device)
    elif grad_fi is False:
        grad_fi = None
    if grad_fi is not None:
        _double_rows(grad_fi, "grad_fi", ncases, no)
    _same_device(g, xk, nk, xi, knowns, weighting_method, grad_fk, grad_fi, case_index)
    s, dev = _stream_and_device(g, stream)
    ci, nsel = _case_index(case_index)
    B.check(B.lib().wlsqm_hip_fit_adjoint_device(C.byref(b), dev, s, int(order), _ptr(g), int(g.stride(0)),
                                                 _ptr(grad_fk), int(grad_fk.stride(0)), int(grad_fk.stride(1)),
                                                 _ptr(grad_fi), int(grad_fi.stride(0)) if grad_fi is not None else 0, ci, nsel))
    return grad_fk, grad_fi


def fit_cloud_adjoint_device(dimension, order, S, hoods, nk, knowns, weighting_method, g, point_index=None, grad_F=None, grad_fi=None,
                             stream=None, slots=None):
    """The vector-Jacobian product of fit_cloud_device: given g (ncases, >= no) = dL/dfi_out, returns (grad_F, grad_fi) =
    (dL/dF (npoints,), dL/dfi_in (ncases, no)).  The kernel runs index-based (xk = S[hoods] is never formed) and writes one gradient
    per neighbour slot, (ncases, K), exact zeros in the padding of a ragged row; one ``index_add_`` then sums the slots into grad_F
    (the padding of `hoods` may hold anything: it is never dereferenced by the kernel and is pointed at point 0 for the scatter).
    grad_F (overwritten) and grad_fi are allocated when not given; grad_fi=False: not wanted; `slots`: a float64 device tensor
    (ncases, K) that receives the per-slot gradients (allocated otherwise).  Asynchronous on `stream`."""
    import torch
    no = _adjoint_order(dimension, order)
    ncases, K = _cloud_geometry(dimension, S, hoods, nk, knowns, weighting_method, point_index,
                                "S must be contiguous; hoods must have a contiguous last axis")
    npoints = int(S.shape[0])
    _double_rows(g, "g", ncases, no)
    if slots is None:
        slots = torch.empty((ncases, K), dtype=torch.float64, device=g.device)
    _double_rows(slots, "slots", ncases, K, says="slots must be at least (ncases, %d) with a contiguous last axis; got %s" % (K, tuple(slots.shape)))
    if grad_fi is None:
        grad_fi = torch.empty((ncases, no), dtype=torch.float64, device=g.device)
    elif grad_fi is False:
        grad_fi = None
    if grad_fi is not None:
        _double_rows(grad_fi, "grad_fi", ncases, no)
    if grad_F is None:
        grad_F = torch.zeros((npoints,), dtype=torch.float64, device=g.device)
    else:
        _check(grad_F, "grad_F", "float64", 1)
        if grad_F.shape[0] < npoints:
            raise ValueError("grad_F has fewer entries than S has points")
    _same_device(g, S, hoods, nk, knowns, weighting_method, point_index, slots, grad_fi, grad_F)
    s, dev = _stream_and_device(g, stream)
    B.check(B.lib().wlsqm_hip_fit_cloud_adjoint_device(int(dimension), int(order), ncases, K, _ptr(S), _ptr(hoods), int(hoods.stride(0)),
                                                       _ptr(point_index), _ptr(nk), _ptr(knowns), _ptr(weighting_method),
                                                       _ptr(g), int(g.stride(0)), _ptr(slots), int(slots.stride(0)),
                                                       _ptr(grad_fi), int(grad_fi.stride(0)) if grad_fi is not None else 0, dev, s))
    # the scatter: torch ops, on the stream of the kernel
    ext = torch.cuda.ExternalStream(int(stream), device=g.device) if stream else None
    with (torch.cuda.stream(ext) if ext is not None else contextlib.nullcontext()):
        live = torch.arange(K, device=g.device)[None, :] < nk[:ncases, None]
        idx = torch.where(live, hoods[:ncases].long(), torch.zeros((), dtype=torch.int64, device=g.device))
        grad_F.zero_()
        grad_F.index_add_(0, idx.reshape(-1), slots[:ncases, :K].reshape(-1))
    return grad_F, grad_fi


# ---- the geometry adjoint of the fit: gradients with respect to the coordinates (csrc/fit_adjoint.hip) ----

def _coordinate_rows(t, name, like, nrows, K, dimension):
    """grad_xk / grad_xi / grad_S: a float64 device tensor of the dimensions of `like` (xk, xi or S) that covers nrows rows, K neighbour
    slots (None: no such axis) and `dimension` contiguous coordinates."""
    _check(t, name, "float64", like.dim())
    if t.shape[0] < nrows:
        raise ValueError(_FEW_ROWS % (name, t.shape[0], nrows))
    if K is not None and t.shape[1] < K:
        raise ValueError("%s has %d neighbour slots per case, fk has %d" % (name, t.shape[1], K))
    if dimension > 1 and (t.stride(-1) != 1 or t.shape[-1] < dimension):
        raise ValueError("%s must have %d contiguous coordinates on the last axis" % (name, dimension))


def fit_many_geometry_adjoint_device(dimension, order, xk, fk, nk, xi, fi_out, knowns, weighting_method, g, grad_xk=None, grad_xi=None,
                                     grad_fk=False, case_index=None, stream=None):
    """The vector-Jacobian product of fit_many_device (basic fit, integer `order`) with respect to the COORDINATES: given
    g (n, >= no) = dL/dfi_out, the arguments of the forward call and fi_out, its output (read, never written), returns
    (grad_xk, grad_xi, grad_fk) = (dL/dxk with xk's shape over the K = fk.shape[1] slots, dL/dxi with xi's shape, dL/dfk (n, K) or None).

    Per case, with d_k = xk_k - xi, c_k the scaled monomials of d_k, phi = fi_out (0 for a DOF dropped by stray high mask bits),
    y_U = M_UU^-1 g_U over the unknowns (0 elsewhere), s_k = c_k . y, r_k = fk_k - c_k . phi and (d_m c) the monomials with the exponent
    on axis m lowered by one:  e[k][m] = (dw_k/dd_k,m) s_k r_k + w_k (r_k (d_m c_k . y) - s_k (d_m c_k . phi));  uniform weights have
    dw = 0, the others dw_k/dd_k,m = -2 beta t_k d_k,m / (rho_k D2) and e[k*][m] += 2 d_k*,m sum_k (beta t_k rho_k / D2) s_k r_k for the
    farthest neighbour k* (beta = 1 - 1e-4, D2 = max d2, rho = sqrt(d2 / D2), t = 1 - rho).  grad_xk[j, k] = e[k] for k < nk[j] and
    exactly 0 for nk[j] <= k; grad_xi[j] = -sum_k e[k]; a case with every DOF known has zeros everywhere.  The fit is not smooth at two
    kinds of point; the conventions: a neighbour ON xi contributes nothing through its weight (the cone of |d| at d = 0 counts as 0),
    and a tie for the farthest neighbour goes to the SMALLEST index (in the kernel's own fp64 squared distances).

    grad_fk: False (not wanted: None is returned), None / True (allocated) or a tensor (n, >= K): dL/dfk = w_k s_k from the same pass,
    for the systems up to 10 unknowns the bits of fit_many_adjoint_device's.  dL/dfi_in stays with fit_many_adjoint_device.  The
    outputs are allocated when not given (with `case_index`: zero-filled, the kernel writes the selected rows only) and must not alias an
    input.  One kernel launch on `stream` (default: torch's current stream), no allocation when the outputs are given, no
    synchronisation: it can be captured.  The arithmetic is always the fast kernels'; hand it the fi_out of the forward call whatever
    mode that ran in.  3D orders 3 and 4 are not covered (ValueError)."""
    import torch
    _adjoint_order(dimension, order)
    no = _ndofs(dimension, order)
    b = _batch(dimension, order, xk, fk, nk, xi, fi_out, knowns, weighting_method, None, False, 0, nk)
    ncases, K = b.ncases, int(fk.shape[1])
    _double_rows(g, "g", ncases, no)
    new = torch.zeros if case_index is not None else torch.empty
    if grad_xk is None:
        grad_xk = new((ncases, K) + tuple(xk.shape[2:]), dtype=torch.float64, device=g.device)
    _coordinate_rows(grad_xk, "grad_xk", xk, ncases, K, dimension)
    if grad_xi is None:
        grad_xi = new((ncases,) + tuple(xi.shape[1:]), dtype=torch.float64, device=g.device)
    _coordinate_rows(grad_xi, "grad_xi", xi, ncases, None, dimension)
    if grad_fk is False:
        grad_fk = None
    elif grad_fk is None or grad_fk is True:
        grad_fk = new((ncases, K), dtype=torch.float64, device=g.device)
    if grad_fk is not None:
        _check(grad_fk, "grad_fk", "float64", 2)
        _rows(ncases, grad_fk=grad_fk)
        if grad_fk.shape[1] < K:
            raise ValueError("grad_fk has %d neighbour slots per case, fk has %d" % (grad_fk.shape[1], K))
    _same_device(g, xk, fk, nk, xi, fi_out, knowns, weighting_method, grad_xk, grad_xi, grad_fk, case_index)
    s, dev = _stream_and_device(g, stream)
    ci, nsel = _case_index(case_index)
    gfk_strides = (int(grad_fk.stride(0)), int(grad_fk.stride(1))) if grad_fk is not None else (0, 0)
    B.check(B.lib().wlsqm_hip_fit_geometry_adjoint_device(C.byref(b), dev, s, int(order), _ptr(g), int(g.stride(0)),
                                                          _ptr(grad_xk), int(grad_xk.stride(0)), int(grad_xk.stride(1)),
                                                          _ptr(grad_xi), int(grad_xi.stride(0)),
                                                          _ptr(grad_fk), gfk_strides[0], gfk_strides[1], ci, nsel))
    return grad_xk, grad_xi, grad_fk


def fit_cloud_geometry_adjoint_device(dimension, order, S, F, hoods, fi_out, nk, knowns, weighting_method, g, point_index=None,
                                      grad_S=None, grad_F=False, stream=None, slots=None, own=None, slots_F=None):
    """The vector-Jacobian product of fit_cloud_device with respect to the point table S: given g (ncases, >= no) = dL/dfi_out, the
    arguments of the forward call and fi_out, its output, returns (grad_S, grad_F) = (dL/dS with S's shape, dL/dF (npoints,) or None).
    The formula and the conventions at the two non-smooth points are fit_many_geometry_adjoint_device's.  The kernel runs index-based
    and writes per case one gradient per neighbour slot, (ncases, K, dim), exact zeros in the padding of a ragged row, and the gradient
    of the case's own point, (ncases, dim); two ``index_add_`` on the kernel's stream then sum them into grad_S: the slots go to
    `hoods` (whose padding may hold anything: it is pointed at point 0, where it adds exact zeros), the own-point rows to `point_index`
    (default: point j).  grad_S (overwritten) is allocated when not given.  grad_F: False (not wanted), None / True (allocated) or a
    tensor (npoints,): dL/dF from the same pass and one more index_add_.  `slots` (ncases, K * dim), `own` (ncases, dim) and `slots_F`
    (ncases, K): float64 device tensors that receive what the kernel writes (allocated otherwise).  Asynchronous on `stream`."""
    import torch
    _adjoint_order(dimension, order)
    no = _ndofs(dimension, order)
    a = _cloud_args(dimension, order, S, F, hoods, fi_out, nk, knowns, weighting_method, point_index)
    ncases, K, npoints = a[2], a[3], int(S.shape[0])
    _double_rows(g, "g", ncases, no)
    z = lambda *shape: torch.empty(shape, dtype=torch.float64, device=g.device)
    if slots is None:
        slots = z(ncases, K * dimension)
    _double_rows(slots, "slots", ncases, K * dimension,
                 says="slots must be at least (ncases, %d) with a contiguous last axis; got %s" % (K * dimension, tuple(slots.shape)))
    if own is None:
        own = z(ncases, dimension)
    _double_rows(own, "own", ncases, dimension,
                 says="own must be at least (ncases, %d) with a contiguous last axis; got %s" % (dimension, tuple(own.shape)))
    if grad_S is None:
        grad_S = torch.zeros(tuple(S.shape), dtype=torch.float64, device=g.device)
    else:
        _check(grad_S, "grad_S", "float64", S.dim())
        if tuple(grad_S.shape) != tuple(S.shape) or not grad_S.is_contiguous():
            raise ValueError("grad_S must be contiguous with the shape of S, %s; got %s" % (tuple(S.shape), tuple(grad_S.shape)))
    if grad_F is False:
        grad_F = None
    elif grad_F is None or grad_F is True:
        grad_F = torch.zeros((npoints,), dtype=torch.float64, device=g.device)
    if grad_F is not None:
        _check(grad_F, "grad_F", "float64", 1)
        if grad_F.shape[0] < npoints:
            raise ValueError("grad_F has fewer entries than S has points")
        if slots_F is None:
            slots_F = z(ncases, K)
        _double_rows(slots_F, "slots_F", ncases, K,
                     says="slots_F must be at least (ncases, %d) with a contiguous last axis; got %s" % (K, tuple(slots_F.shape)))
    else:
        slots_F = None
    _same_device(g, S, F, hoods, nk, fi_out, knowns, weighting_method, point_index, slots, own, grad_S, grad_F, slots_F)
    s, dev = _stream_and_device(g, stream)
    B.check(B.lib().wlsqm_hip_fit_cloud_geometry_adjoint_device(*a, _ptr(g), int(g.stride(0)), _ptr(slots), int(slots.stride(0)),
                                                                _ptr(own), int(own.stride(0)), _ptr(slots_F),
                                                                int(slots_F.stride(0)) if slots_F is not None else 0, dev, s))
    # the scatter: torch ops, on the stream of the kernel
    ext = torch.cuda.ExternalStream(int(stream), device=g.device) if stream else None
    with (torch.cuda.stream(ext) if ext is not None else contextlib.nullcontext()):
        live = torch.arange(K, device=g.device)[None, :] < nk[:ncases, None]
        idx = torch.where(live, hoods[:ncases].long(), torch.zeros((), dtype=torch.int64, device=g.device)).reshape(-1)
        pts = point_index[:ncases].long() if point_index is not None else torch.arange(ncases, device=g.device)
        flat = grad_S.view(npoints, dimension)
        flat.zero_()
        flat.index_add_(0, idx, slots[:ncases, :K * dimension].reshape(ncases * K, dimension))
        flat.index_add_(0, pts, own[:ncases, :dimension])
        if grad_F is not None:
            grad_F.zero_()
            grad_F.index_add_(0, idx, slots_F[:ncases, :K].reshape(-1))
    return grad_S, grad_F


# ---- autograd: gradients through the fits, the prepared solver (ExpertSolver.solve_adjoint_device; csrc/solve_op.hip, DESIGN.md
# section 13) and the evaluation of a plan (InterpolationPlan.evaluate_adjoint) ----

_AUTOGRAD = None


def _autograd():
    """The torch.autograd.Function classes behind the differentiable_* functions, as a namespace with FitMany, FitCloud, Solve,
    Evaluate, FitManyGeometry, FitCloudGeometry, StencilApply, StencilSolve, StencilSystemSolve and StencilSolveMany (made at first use: the module does not import torch).  Every forward takes its tensor inputs first."""
    global _AUTOGRAD
    if _AUTOGRAD is not None:
        return _AUTOGRAD
    import types
    import torch
    from torch.autograd.function import once_differentiable

    def gradients(ctx, gout, ntensors, adjoint):
        """The frame of every backward pass: one entry per input of the forward, None for all of them when no tensor input wants
        a gradient (nothing is launched), else what adjoint(g, *wanted) returns for the tensor inputs that want theirs."""
        wanted = ctx.needs_input_grad[:ntensors]
        out = [None] * len(ctx.needs_input_grad)
        if any(wanted):
            for i, grad in enumerate(adjoint(gout.contiguous(), *wanted)):
                if wanted[i]:
                    out[i] = grad
        return tuple(out)

    def buffer(shape, g, covered):
        """A gradient the adjoint kernel writes into: uninitialised when the kernel covers every element of it, zeros otherwise."""
        return (torch.empty if covered else torch.zeros)(shape, dtype=torch.float64, device=g.device)

    def grad_fi_start(g, wanted, covered):
        """The grad_fi argument of an in-place fit's adjoint: False when not wanted; a copy of g when fi has rows or columns the
        forward never touches (they leave as they came in, so dL/dfi_in is g there); None (the adjoint allocates) otherwise."""
        if not wanted:
            return False
        return None if covered else g.clone()

    class FitMany(torch.autograd.Function):
        @staticmethod
        def forward(ctx, fk, fi, dimension, order, xk, nk, xi, knowns, weighting_method, strict, stream):
            out = fi.detach().clone()
            fit_many_device(dimension, order, xk, fk.detach(), nk, xi, out, knowns, weighting_method, strict=strict, stream=stream)
            ctx.geometry = (dimension, order, xk, nk, xi, knowns, weighting_method, stream, tuple(fk.shape))
            return out

        @staticmethod
        @once_differentiable
        def backward(ctx, gout):
            def adjoint(g, need_fk, need_fi):
                dimension, order, xk, nk, xi, knowns, weighting_method, stream, fk_shape = ctx.geometry
                ncases, K, no = int(nk.shape[0]), int(fk_shape[1]), _ndofs(dimension, order)
                gfk = buffer(fk_shape, g, fk_shape[0] == ncases)
                gfi = grad_fi_start(g, need_fi, g.shape[0] == ncases and g.shape[1] == no)
                return fit_many_adjoint_device(dimension, order, xk[:, :K], nk, xi, knowns, weighting_method, g, grad_fk=gfk,
                                               grad_fi=gfi, stream=stream)
            return gradients(ctx, gout, 2, adjoint)

    class FitCloud(torch.autograd.Function):
        @staticmethod
        def forward(ctx, F, fi, dimension, order, S, hoods, nk, knowns, weighting_method, point_index, strict, stream):
            out = fi.detach().clone()
            fit_cloud_device(dimension, order, S, F.detach(), hoods, out, nk, knowns, weighting_method, point_index=point_index,
                             strict=strict, stream=stream)
            ctx.geometry = (dimension, order, S, hoods, nk, knowns, weighting_method, point_index, stream, tuple(F.shape))
            return out

        @staticmethod
        @once_differentiable
        def backward(ctx, gout):
            def adjoint(g, need_F, need_fi):
                dimension, order, S, hoods, nk, knowns, weighting_method, point_index, stream, F_shape = ctx.geometry
                gF = buffer(F_shape, g, True)
                gfi = grad_fi_start(g, need_fi, g.shape[0] == int(hoods.shape[0]) and g.shape[1] == _ndofs(dimension, order))
                return fit_cloud_adjoint_device(dimension, order, S, hoods, nk, knowns, weighting_method, g, point_index=point_index,
                                                grad_F=gF, grad_fi=gfi, stream=stream)
            return gradients(ctx, gout, 2, adjoint)

    class Solve(torch.autograd.Function):
        @staticmethod
        def forward(ctx, fk, fi, solver, stream, many):
            out = fi.detach().clone()
            (solver.solve_many_device if many else solver.solve_device)(fk.detach(), out, stream=stream)
            ctx.call = (solver, stream, many, tuple(fk.shape), tuple(fi.shape))
            return out

        @staticmethod
        @once_differentiable
        def backward(ctx, gout):
            def adjoint(g, need_fk, need_fi):
                solver, stream, many, fk_shape, fi_shape = ctx.call
                # rows beyond ncases receive no gradient (the columns beyond the solver's slots are zero-filled by the call itself)
                gfk = buffer(fk_shape, g, fk_shape[-2] == solver.ncases)
                gfi = grad_fi_start(g, need_fi, need_fi and fi_shape[-2] == solver.ncases and fi_shape[-1] == solver._max_no
                                    and solver.uniform_order)
                return (solver.solve_many_adjoint_device if many else solver.solve_adjoint_device)(g, grad_fk=gfk, grad_fi=gfi,
                                                                                                   stream=stream)
            return gradients(ctx, gout, 2, adjoint)

    class Evaluate(torch.autograd.Function):
        @staticmethod
        def forward(ctx, fi, plan, diff, stream):
            ctx.call = (plan, diff, stream, tuple(fi.shape))
            return plan.evaluate(diff, fi.detach(), stream=stream)

        @staticmethod
        @once_differentiable
        def backward(ctx, gout):
            def adjoint(g, need_fi):
                plan, diff, stream, fi_shape = ctx.call
                # rows beyond nmodels and columns beyond the plan's DOFs are never read by the forward: zeros
                gfi = buffer(fi_shape, g, fi_shape[-2] == plan.nmodels and fi_shape[-1] == plan._max_no)
                return (plan.evaluate_adjoint(g, diff, grad_fi=gfi, stream=stream),)
            return gradients(ctx, gout, 1, adjoint)

    class FitManyGeometry(torch.autograd.Function):
        """FitMany with the coordinates among the differentiable inputs: saves fk and the output for the geometry adjoint."""
        @staticmethod
        def forward(ctx, xk, xi, fk, fi, dimension, order, nk, knowns, weighting_method, strict, stream):
            out = fi.detach().clone()
            fit_many_device(dimension, order, xk.detach(), fk.detach(), nk, xi.detach(), out, knowns, weighting_method, strict=strict,
                            stream=stream)
            ctx.save_for_backward(xk, xi, fk, out)
            ctx.geometry = (dimension, order, nk, knowns, weighting_method, stream)
            return out

        @staticmethod
        @once_differentiable
        def backward(ctx, gout):
            def adjoint(g, need_xk, need_xi, need_fk, need_fi):
                dimension, order, nk, knowns, weighting_method, stream = ctx.geometry
                xk, xi, fk, out = ctx.saved_tensors
                ncases, K, no = int(nk.shape[0]), int(fk.shape[1]), _ndofs(dimension, order)
                gxk = gxi = gfk = gfi = None
                if need_xk or need_xi:
                    # the geometry kernel; dL/dfk, when wanted, is its fused output
                    gxk = buffer(tuple(xk.shape), g, xk.shape[0] == ncases and xk.shape[1] == K and (xk.dim() == 2 or xk.shape[2] == dimension))
                    gxi = buffer(tuple(xi.shape), g, xi.shape[0] == ncases and (xi.dim() == 1 or xi.shape[1] == dimension))
                    gfk = buffer(tuple(fk.shape), g, fk.shape[0] == ncases) if need_fk else False
                    _, _, gfk = fit_many_geometry_adjoint_device(dimension, order, xk, fk, nk, xi, out, knowns, weighting_method, g,
                                                                 grad_xk=gxk, grad_xi=gxi, grad_fk=gfk, stream=stream)
                    need_fk = False
                if need_fk or need_fi:
                    # the existing adjoint: only when fi wants a gradient, or fk alone does
                    scratch = buffer(tuple(fk.shape), g, fk.shape[0] == ncases)
                    got, gfi = fit_many_adjoint_device(dimension, order, xk[:, :K], nk, xi, knowns, weighting_method, g, grad_fk=scratch,
                                                       grad_fi=grad_fi_start(g, need_fi, g.shape[0] == ncases and g.shape[1] == no),
                                                       stream=stream)
                    gfk = got if need_fk else gfk
                return gxk, gxi, gfk, gfi
            return gradients(ctx, gout, 4, adjoint)

    class FitCloudGeometry(torch.autograd.Function):
        """FitCloud with the point table among the differentiable inputs."""
        @staticmethod
        def forward(ctx, S, F, fi, dimension, order, hoods, nk, knowns, weighting_method, point_index, strict, stream):
            out = fi.detach().clone()
            fit_cloud_device(dimension, order, S.detach(), F.detach(), hoods, out, nk, knowns, weighting_method, point_index=point_index,
                             strict=strict, stream=stream)
            ctx.save_for_backward(S, F, out)
            ctx.geometry = (dimension, order, hoods, nk, knowns, weighting_method, point_index, stream)
            return out

        @staticmethod
        @once_differentiable
        def backward(ctx, gout):
            def adjoint(g, need_S, need_F, need_fi):
                dimension, order, hoods, nk, knowns, weighting_method, point_index, stream = ctx.geometry
                S, F, out = ctx.saved_tensors
                gS = gF = gfi = None
                if need_S:
                    gS, gF = fit_cloud_geometry_adjoint_device(dimension, order, S, F, hoods, out, nk, knowns, weighting_method, g,
                                                               point_index=point_index, grad_F=buffer(tuple(F.shape), g, True) if need_F else False,
                                                               stream=stream)
                    need_F = False
                if need_F or need_fi:
                    covered = g.shape[0] == int(hoods.shape[0]) and g.shape[1] == _ndofs(dimension, order)
                    got, gfi = fit_cloud_adjoint_device(dimension, order, S, hoods, nk, knowns, weighting_method, g, point_index=point_index,
                                                        grad_F=buffer(tuple(F.shape), g, True), grad_fi=grad_fi_start(g, need_fi, covered),
                                                        stream=stream)
                    gF = got if need_F else gF
                return gS, gF, gfi
            return gradients(ctx, gout, 3, adjoint)

    class StencilApply(torch.autograd.Function):
        @staticmethod
        def forward(ctx, F, known, op, stream):
            ctx.call = (op, stream, tuple(F.shape), tuple(known.shape) if known is not None else None)
            return op.apply(F.detach(), known=known.detach() if known is not None else None, stream=stream)

        @staticmethod
        @once_differentiable
        def backward(ctx, gout):
            def adjoint(g, need_F, need_known):
                op, stream, F_shape, known_shape = ctx.call
                gF = gknown = None
                if need_F:
                    # entries of F beyond the operator's points are never read by the forward: zeros
                    gF = buffer(F_shape, g, F_shape[-1] == op.npoints)
                    op.apply_transpose(g, out=gF[..., :op.npoints], stream=stream)
                if need_known:
                    gknown = op._known_adjoint(g, known_shape, stream)
                return gF, gknown
            return gradients(ctx, gout, 2, adjoint)

    class StencilSolve(torch.autograd.Function):
        """StencilSolver.solve with b, the diag tensor, the point table and the coefficients among the differentiable inputs."""
        @staticmethod
        def forward(ctx, b, diag, S, slots, own, x0, solver, rtol, atol, maxiter, check_every, adjoint_rtol, stream):
            op = solver._op
            det = lambda t: t.detach() if t is not None else None
            if S is not None:
                op.update(S.detach(), stream=stream)
            if slots is not None:
                op.set_coefficients(slots.detach(), det(own), stream=stream)
            with _torch_stream(stream, solver._device):
                x = x0.detach().clone() if x0 is not None else torch.zeros((solver.npoints,), dtype=torch.float64, device=solver._device)
            info = solver.solve(b.detach(), x, rtol=rtol, atol=atol, maxiter=maxiter, check_every=check_every, stream=stream)
            if info.status != 0:
                raise RuntimeError("the forward solve did not converge: status %d, %r" % (info.status, info))
            ctx.save_for_backward(x, *(t for t in (S, slots, own) if t is not None))
            ctx.call = (solver, S is not None, slots is not None, own is not None, adjoint_rtol if adjoint_rtol is not None else rtol,
                        maxiter, check_every, stream)
            return x

        @staticmethod
        @once_differentiable
        def backward(ctx, gout):
            def adjoint(g, need_b, need_diag, need_S, need_slots, need_own):
                solver, has_S, has_slots, has_own, rtol, maxiter, check_every, stream = ctx.call
                x, *made_from = ctx.saved_tensors
                op, o, device = solver._op, solver._o, solver._device
                solver._no_capture("the backward pass of differentiable_stencil_solve", stream)
                if has_S:                                    # the operator back where the forward had it
                    op.update(made_from[0].detach(), check=False, stream=stream)
                elif has_slots:
                    op.set_coefficients(made_from[0].detach(), made_from[1].detach() if has_own else None, stream=stream)
                with _torch_stream(stream, device):
                    lam = torch.zeros((solver.npoints,), dtype=torch.float64, device=device)
                    x = x.detach()
                info = solver.solve(g, lam, rtol=rtol, atol=0.0, maxiter=maxiter, check_every=check_every, stream=stream, transpose=True)
                if info.status != 0:
                    raise RuntimeError("the adjoint solve did not converge: status %d, %r" % (info.status, info))
                gdiag = gS = gslots = gown = None
                if need_diag or need_slots or need_own:
                    got = solver.gradients(lam, x, values=need_slots or need_own, diag=need_diag, stream=stream)
                    gdiag = got.diag
                    if got.values is not None:
                        with _torch_stream(stream, device):
                            sl, ow = op.unpack(got.values)
                            if need_slots:
                                gslots = torch.zeros(tuple(made_from[0].shape), dtype=torch.float64, device=device)
                                gslots[o, :op.ncases, :op.K] = sl
                            if need_own:
                                gown = torch.zeros(tuple(made_from[1].shape), dtype=torch.float64, device=device)
                                gown[o, :op.ncases] = ow
                if need_S:
                    gS = _solve_geometry_adjoint(solver, made_from[0].detach(), x, lam, stream)
                return lam, gdiag, gS, gslots, gown
            return gradients(ctx, gout, 5, adjoint)

    class StencilSystemSolve(torch.autograd.Function):
        """StencilSystemSolver.solve with b, the diag tensor, the point table, the coefficients and coupling among the differentiable
        inputs."""
        @staticmethod
        def forward(ctx, b, diag, S, slots, own, coupling, x0, solver, rtol, atol, maxiter, check_every, adjoint_rtol, stream):
            op = solver._op
            det = lambda t: t.detach() if t is not None else None
            if S is not None:
                op.update(S.detach(), stream=stream)
            if slots is not None:
                op.set_coefficients(slots.detach(), det(own), stream=stream)
            if coupling is not None:
                solver.set_coupling(coupling.detach() if solver.per_point else coupling.detach().cpu().numpy())
            with _torch_stream(stream, solver._device):
                x = (x0.detach().clone() if x0 is not None
                     else torch.zeros((solver.npoints, solver.m), dtype=torch.float64, device=solver._device))
            info = solver.solve(b.detach(), x, rtol=rtol, atol=atol, maxiter=maxiter, check_every=check_every, stream=stream)
            if info.status != 0:
                raise RuntimeError("the forward solve did not converge: status %d, %r" % (info.status, info))
            ctx.save_for_backward(x, *(t for t in (S, slots, own, coupling) if t is not None))
            ctx.call = (solver, S is not None, slots is not None, own is not None, coupling is not None,
                        adjoint_rtol if adjoint_rtol is not None else rtol, maxiter, check_every, stream)
            return x

        @staticmethod
        @once_differentiable
        def backward(ctx, gout):
            def adjoint(g, need_b, need_diag, need_S, need_slots, need_own, need_coupling):
                solver, has_S, has_slots, has_own, has_coupling, rtol, maxiter, check_every, stream = ctx.call
                x, *made_from = ctx.saved_tensors
                op, device = solver._op, solver._device
                solver._no_capture("the backward pass of differentiable_stencil_system_solve", stream)
                cp = made_from.pop() if has_coupling else None
                if has_S:                                    # the operator and coupling back where the forward had them
                    op.update(made_from[0].detach(), check=False, stream=stream)
                elif has_slots:
                    op.set_coefficients(made_from[0].detach(), made_from[1].detach() if has_own else None, stream=stream)
                if has_coupling:
                    solver.set_coupling(cp.detach() if solver.per_point else cp.detach().cpu().numpy())
                with _torch_stream(stream, device):
                    lam = torch.zeros((solver.npoints, solver.m), dtype=torch.float64, device=device)
                    x = x.detach()
                info = solver.solve(g, lam, rtol=rtol, atol=0.0, maxiter=maxiter, check_every=check_every, stream=stream, transpose=True)
                if info.status != 0:
                    raise RuntimeError("the adjoint solve did not converge: status %d, %r" % (info.status, info))
                gdiag = gS = gslots = gown = gcp = None
                if need_diag or need_slots or need_own:
                    got = solver.gradients(lam, x, values=need_slots or need_own, diag=need_diag, stream=stream)
                    gdiag = got.diag
                    if got.values is not None:
                        with _torch_stream(stream, device):
                            sl, ow = op._unpack(got.values)
                            if need_slots:
                                gslots = torch.zeros(tuple(made_from[0].shape), dtype=torch.float64, device=device)
                                gslots[:, :op.ncases, :op.K] = sl
                            if need_own:
                                gown = torch.zeros(tuple(made_from[1].shape), dtype=torch.float64, device=device)
                                gown[:op.nop, :op.ncases] = ow
                if need_S:
                    gS = _system_geometry_adjoint(solver, made_from[0].detach(), x, lam, stream)
                if need_coupling:
                    gcp = solver.coupling_gradient(lam, x, stream=stream).to(cp.device)
                return lam, gdiag, gS, gslots, gown, gcp
            return gradients(ctx, gout, 6, adjoint)

    class StencilSolveMany(torch.autograd.Function):
        """StencilSolver.solve_many as a differentiable function of b alone: the backward pass is one solve_many(transpose=True) on the
        incoming gradient.  The gradients with respect to the operator (S, the coefficients), diag and scale are out of scope for
        stacked solves: take them field by field through differentiable_stencil_solve."""
        @staticmethod
        def forward(ctx, b, x0, solver, rtol, atol, maxiter, check_every, adjoint_rtol, stream):
            with _torch_stream(stream, solver._device):
                x = (x0.detach().clone(memory_format=torch.contiguous_format) if x0 is not None
                     else torch.zeros((solver.nfields, solver.npoints), dtype=torch.float64, device=solver._device))
            infos = solver.solve_many(b.detach(), x, rtol=rtol, atol=atol, maxiter=maxiter, check_every=check_every, stream=stream)
            if any(info.status != 0 for info in infos):
                raise RuntimeError("the forward solve did not converge: %r" % (infos,))
            ctx.call = (solver, adjoint_rtol if adjoint_rtol is not None else rtol, maxiter, check_every, stream)
            return x

        @staticmethod
        @once_differentiable
        def backward(ctx, gout):
            def adjoint(g, need_b):
                solver, rtol, maxiter, check_every, stream = ctx.call
                solver._no_capture("the backward pass of differentiable_stencil_solve_many", stream)
                with _torch_stream(stream, solver._device):
                    lam = torch.zeros((solver.nfields, solver.npoints), dtype=torch.float64, device=solver._device)
                infos = solver.solve_many(g, lam, rtol=rtol, atol=0.0, maxiter=maxiter, check_every=check_every, stream=stream,
                                          transpose=True)
                if any(info.status != 0 for info in infos):
                    raise RuntimeError("the adjoint solve did not converge: %r" % (infos,))
                return (lam,)
            return gradients(ctx, gout, 1, adjoint)

    _AUTOGRAD = types.SimpleNamespace(FitMany=FitMany, FitCloud=FitCloud, Solve=Solve, Evaluate=Evaluate, FitManyGeometry=FitManyGeometry,
                                      FitCloudGeometry=FitCloudGeometry, StencilApply=StencilApply, StencilSolve=StencilSolve,
                                      StencilSolveMany=StencilSolveMany, StencilSystemSolve=StencilSystemSolve)
    return _AUTOGRAD


def _solve_geometry_adjoint(solver, S, x, lam, stream):
    """dL/dS through M x = b at fixed x, lam and neighbour lists: -scale * lam^T (dA_o) x.  Row j of A_o applied to x is
    rows[o] . fi_out[j] of a fit of F = x, so this is the geometry adjoint of that fit with g_j = -scale * lam_j * rows[o]
    (DESIGN.md section 18): one fit and one geometry-adjoint launch, with the adjoint's two index_add_."""
    import torch
    op = solver._op
    hoods, nk, knowns, weighting_method, point_index = op._geo
    rows, no, n = op._rows, op.no, op.ncases
    with _torch_stream(stream, solver._device):
        if S.shape[0] == op.npoints:
            F = x
        else:                                                # points beyond the operator's: no live entry names them
            F = torch.zeros((S.shape[0],), dtype=torch.float64, device=solver._device)
            F[:op.npoints] = x
        fi = torch.zeros((n, no), dtype=torch.float64, device=solver._device)
        fi[:, 0] = x[:n]                                     # the F-known cases take their own value from here (row j is point j)
        row = rows[solver._o, :n, :no] if rows.dim() == 3 else rows[solver._o, :no][None, :]
        g = ((-solver.scale) * lam[:n])[:, None] * row
    fit_cloud_device(op.dimension, op.order, S, F, hoods, fi, nk, knowns, weighting_method, point_index=point_index, stream=stream)
    return fit_cloud_geometry_adjoint_device(op.dimension, op.order, S, F, hoods, fi, nk, knowns, weighting_method, g.contiguous(),
                                             point_index=point_index, stream=stream)[0]


def _system_geometry_adjoint(solver, S, x, lam, stream):
    """dL/dS through the coupled M x = b at fixed x, lam and neighbour lists: section 18's route once per
    component b — the fit of F = x[:, b] and its geometry adjoint with g_j = -sum_o (sum_a coupling[a, b, o] lam[j, a]) rows[o], per-case
    rows where the operator has them — and the m results summed in component order.  A per-point table (section 26) contributes
    coupling[a, b, o, j], the coefficients of row j."""
    import torch
    op = solver._op
    hoods, nk, knowns, weighting_method, point_index = op._geo
    rows, no, n = op._rows, op.no, op.ncases
    total = None
    for b in range(solver.m):
        with _torch_stream(stream, solver._device):
            if solver.per_point:                             # u[j, o] = sum_a coupling[a, b, o, j] lam[j, a]
                u = torch.einsum("aoj,ja->jo", solver.coupling[:, b, :, :n], lam[:n])
            else:
                cp = torch.from_numpy(solver.coupling[:, b, :].copy()).to(solver._device)      # (m, nop): coupling[a, b, o]
                u = lam[:n] @ cp                                                               # (n, nop)
            F = torch.zeros((S.shape[0],), dtype=torch.float64, device=solver._device)         # points beyond the operator's: never named
            F[:op.npoints] = x[:, b]
            fi = torch.zeros((n, no), dtype=torch.float64, device=solver._device)
            fi[:, 0] = x[:n, b]                              # the F-known cases take their own value from here (row j is point j)
            g = -(torch.einsum("jo,ojn->jn", u, rows[:, :n, :no]) if rows.dim() == 3 else u @ rows[:, :no])
        fit_cloud_device(op.dimension, op.order, S, F, hoods, fi, nk, knowns, weighting_method, point_index=point_index, stream=stream)
        part = fit_cloud_geometry_adjoint_device(op.dimension, op.order, S, F, hoods, fi, nk, knowns, weighting_method, g.contiguous(),
                                                 point_index=point_index, stream=stream)[0]
        with _torch_stream(stream, solver._device):
            total = part if total is None else total.add_(part)
    return total


def _no_geometry_grad(*geometry):
    """The tensors a fit's geometry is made of, or a plan (which remembers whether the tensors it was made from required one)."""
    for t in geometry:
        if t is not None and (getattr(t, "requires_grad", False) or getattr(t, "_geometry_requires_grad", False)):
            raise ValueError("the geometry is not differentiable")


def differentiable_fit_many(dimension, order, xk, fk, nk, xi, fi, knowns, weighting_method, strict=None, stream=None, geometry=False):
    """fit_many_device as a differentiable function of fk and fi: returns fi_out, a NEW tensor (fi is cloned, the fit runs in place on
    the clone), through which autograd reaches fk and fi (the basic fit, integer `order`; refinement is not offered: its stop test
    is data-dependent).  The backward pass is fit_many_adjoint_device: one kernel, computed only for the inputs that require a gradient;
    it always runs the fast arithmetic, whatever `strict` the forward used.  The geometry (xk, xi) is not differentiable:
    ValueError when it requires a gradient.  Once differentiable.

    geometry=True: a differentiable function of the coordinates xk and xi as well.  The backward pass runs
    fit_many_geometry_adjoint_device for xk and xi (dL/dfk, when wanted too, is its fused output) and fit_many_adjoint_device only
    when fi wants a gradient (or fk alone does); nothing is launched for inputs that need none.  The conventions at the fit's two
    non-smooth points (a neighbour on xi, a tie for the farthest neighbour) are fit_many_geometry_adjoint_device's.  Once differentiable."""
    _adjoint_order(dimension, order)
    if geometry:
        return _autograd().FitManyGeometry.apply(xk, xi, fk, fi, dimension, int(order), nk, knowns, weighting_method, strict, stream)
    _no_geometry_grad(xk, xi)
    return _autograd().FitMany.apply(fk, fi, dimension, int(order), xk, nk, xi, knowns, weighting_method, strict, stream)


def differentiable_fit_cloud(dimension, order, S, F, hoods, fi, nk, knowns, weighting_method, point_index=None, strict=None, stream=None,
                             geometry=False):
    """fit_cloud_device as a differentiable function of the field F (npoints,) and of fi: returns fi_out, a new tensor.  The backward
    pass is fit_cloud_adjoint_device (index-based kernel + one index_add_ into dL/dF).  S is not differentiable (ValueError).
    geometry=True: a differentiable function of the point table S as well, through fit_cloud_geometry_adjoint_device (dL/dF, when wanted
    too, from the same kernel; fit_cloud_adjoint_device only when fi wants a gradient or F alone does)."""
    _adjoint_order(dimension, order)
    if geometry:
        return _autograd().FitCloudGeometry.apply(S, F, fi, dimension, int(order), hoods, nk, knowns, weighting_method, point_index, strict,
                                                  stream)
    _no_geometry_grad(S)
    return _autograd().FitCloud.apply(F, fi, dimension, int(order), S, hoods, nk, knowns, weighting_method, point_index, strict, stream)


def _differentiable_solve(solver, fk, fi, stream, many):
    solver._check_tensors(3 if many else 2, ("fk", "fi"), ((fk, "fk"),), ((fi, "fi"),))      # before anything is cloned
    return _autograd().Solve.apply(fk, fi, solver, stream, many)


def differentiable_solve(solver, fk, fi, stream=None):
    """ExpertSolver.solve_device as a differentiable function of fk (ncases, >= max_nk) and fi (ncases, >= no) on the prepared
    geometry of `solver`: returns fi_out, a NEW tensor (fi is cloned and the in-place solve runs on the clone, so the solver's
    "latest solve" that interpolate() evaluates is the returned tensor).  The backward pass is solver.solve_adjoint_device, computed
    only for the inputs that require a gradient; dL/dfk has fk's full shape (zeros in rows and columns the solve never reads), rows
    and columns of fi that the solve never touches pass the incoming gradient through.  ALGO_BASIC solvers only.  Once differentiable."""
    return _differentiable_solve(solver, fk, fi, stream, False)


def differentiable_solve_many(solver, fk, fi, stream=None):
    """ExpertSolver.solve_many_device as a differentiable function of fk (nrhs, ncases, >= max_nk) and fi (nrhs, ncases, >= no): see
    differentiable_solve.  The backward pass is solver.solve_many_adjoint_device: with the stored solution operator present
    (solver.prepare_operator()) one batched GEMM with its transpose for the whole stack."""
    return _differentiable_solve(solver, fk, fi, stream, True)


def knn(S, k, stream=None, nquery=None):
    """The k nearest OTHER points of every point of the device-resident cloud S (npoints, dim) [1D: (npoints,)], as an
    int32 device tensor (npoints, k), ascending by (distance, index) — what the reference's examples get on the host from
    ``cKDTree(S).query(S, 1 + k)[1][:, 1:]`` (examples/expertsolver_example.py:48-66).  Exact uniform-grid search on the
    GPU; the result is the ``hoods`` argument of fit_cloud_device / ShardedCloudSolver, or of ``S[hoods]`` for the dense
    API.  1 <= k <= min(npoints - 1, 213).  Synchronises the stream.
    With `nquery`, only the first nquery points ask and the rest are candidates only: returns (nquery, k).
    Domain: finite coordinates (a NaN or an infinity anywhere in S raises ValueError) whose bounding box has a representable squared
    diagonal (ValueError otherwise); squared distances must not underflow either (points closer than about 2^-511 on every axis
    count as coincident).  Coincident points are legal.  Equal distances are ordered by index; where a tie straddles the k-th
    place, which of its members fill the last slots is not specified."""
    import torch
    if S.dim() == 1:
        dim = 1
    elif S.dim() == 2 and 1 <= S.shape[1] <= 3:
        dim = int(S.shape[1])
    else:
        raise ValueError("S must be (npoints,) or (npoints, dim) with dim 1..3")
    _check(S, "S", "float64", S.dim())
    if not S.is_contiguous():
        raise ValueError("S must be contiguous")
    n = int(S.shape[0])
    nq = n if nquery is None else int(nquery)
    if not 0 < nq <= n:
        raise ValueError("nquery must be in 1 .. npoints")
    hoods = torch.empty((nq, int(k)), dtype=torch.int32, device=S.device)
    s, dev = _stream_and_device(S, stream)
    if nquery is None:
        B.check(B.lib().wlsqm_hip_knn_device(dim, n, _ptr(S), int(k), _ptr(hoods), dev, s))
    else:
        B.check(B.lib().wlsqm_hip_knn_subset_device(dim, n, _ptr(S), int(k), nq, _ptr(hoods), dev, s))
    return hoods


def ball(S, radius, max_nk, stream=None):
    """All OTHER points within `radius` of every point of the device-resident cloud S, nearest first, at most max_nk of
    them: returns (hoods, nk) = int32 device tensors (npoints, max_nk) and (npoints,).  The radius form of knn(): what
    the reference's examples/wlsqm_example.py:103-133 builds with ``cKDTree.query_ball_point`` (unused slots of a row
    hold the point's own index, so the rows stay valid for fit_cloud_device with the returned nk).
    The ball is closed (squared distance <= radius * radius, both as computed in float64) and the row ascends by (distance, index);
    radius > 0, and S in the domain of knn().  Of a ball with more than max_nk members the max_nk nearest are kept (nk == max_nk)."""
    import torch
    dim = 1 if S.dim() == 1 else int(S.shape[1])
    if S.dim() not in (1, 2) or not 1 <= dim <= 3:
        raise ValueError("S must be (npoints,) or (npoints, dim) with dim 1..3")
    _check(S, "S", "float64", S.dim())
    if not S.is_contiguous():
        raise ValueError("S must be contiguous")
    n = int(S.shape[0])
    hoods = torch.empty((n, int(max_nk)), dtype=torch.int32, device=S.device)
    nk = torch.empty((n,), dtype=torch.int32, device=S.device)
    s, dev = _stream_and_device(S, stream)
    B.check(B.lib().wlsqm_hip_ball_device(dim, n, _ptr(S), float(radius), int(max_nk), _ptr(hoods), _ptr(nk), dev, s))
    return hoods, nk


def nearest(S, X, stream=None):
    """Index (int64 device tensor, one per row of X) of the point of the device-resident cloud S nearest to each query
    point X[j] (queries need not belong to the cloud; ties go to the smaller index): ``cKDTree(S).query(X)[1]`` on the GPU.
    S in the domain of knn().  A query with a NaN coordinate, or one so far away that its squared distances overflow, has no nearest
    point and gets 2**31 - 1, which is no index of S (a plan evaluates to NaN there)."""
    import torch
    dim = 1 if S.dim() == 1 else int(S.shape[1])
    _check(S, "S", "float64", S.dim()); _check(X, "X", "float64", X.dim())
    if not S.is_contiguous() or not X.is_contiguous() or (1 if X.dim() == 1 else int(X.shape[1])) != dim:
        raise ValueError("S and X must be contiguous and have the same number of coordinates")
    out = torch.empty((int(X.shape[0]),), dtype=torch.int64, device=S.device)
    s, dev = _stream_and_device(S, stream)
    B.check(B.lib().wlsqm_hip_nearest_device(dim, int(S.shape[0]), _ptr(S), int(X.shape[0]), _ptr(X), dim, _ptr(out), dev, s))
    return out


def grid_shape(dimension, npoints, lo, hi):
    """(g, cell): the cells per axis (int32 array) and their sides (float64 array) of the uniform grid that knn, ball, nearest and the
    continuous interpolation lay over a cloud of npoints points with the bounding box lo .. hi.  Host arithmetic only (no device is
    touched); ValueError for a box outside the searches' domain (see knn)."""
    import numpy as np
    dimension = int(dimension)
    lo = np.ascontiguousarray(np.atleast_1d(lo), dtype=np.float64)
    hi = np.ascontiguousarray(np.atleast_1d(hi), dtype=np.float64)
    if dimension not in (1, 2, 3) or lo.shape != (dimension,) or hi.shape != (dimension,):
        raise ValueError("lo and hi must hold `dimension` = 1..3 numbers each")
    g = np.ones(dimension, np.int32)
    cell = np.ones(dimension, np.float64)
    B.check(B.lib().wlsqm_hip_grid_shape_host(dimension, int(npoints), lo.ctypes.data, hi.ctypes.data, g.ctypes.data, cell.ctypes.data))
    return g, cell


# ---- the Morton order of a cloud, and everything renumbered with it (csrc/order.hip) ----

def _cloud_dim(S):
    """The dimension of a cloud S (npoints,) or (npoints, dim), checked as knn checks it."""
    if not hasattr(S, "dim") or not hasattr(S, "is_cuda"):
        raise ValueError("argument S must be a device (HIP) tensor")
    if S.dim() == 1:
        dim = 1
    elif S.dim() == 2 and 1 <= S.shape[1] <= 3:
        dim = int(S.shape[1])
    else:
        raise ValueError("S must be (npoints,) or (npoints, dim) with dim 1..3")
    _check(S, "S", "float64", S.dim())
    if not S.is_contiguous():
        raise ValueError("S must be contiguous")
    return dim


class SpatialOrder:
    """The Morton order of a device-resident cloud S (npoints, dim) [1D: (npoints,)], dim 1..3: what the
    index-based fits, StencilOperator.apply, the Krylov kernels and a BlockJacobi want the points to be numbered by, for a cloud that
    comes in any other order — with the renumbering of everything that names points.

    2D / 3D: per axis q = min(floor(((x - lo) / (hi - lo)) * 2^B), 2^B - 1) with B = 31 / 21 bits (0 on an axis without extent), the
    bits of the axes interleaved (axis 0 lowest) into a non-negative int64 key; 1D: the exact order of the doubles.  `perm` is the
    stable ascending sort of the keys (ties go to the smaller old index): new position i holds old point perm[i], and
    inverse[perm[i]] = i.  The order is monotone per axis and does not change when the cloud is scaled by a power of two;
    tests/_order_ref.py states it in numpy and the device reproduces it bit for bit.

    S in the domain of knn (a NaN or an infinity raises ValueError, as does a box whose squared diagonal overflows); npoints >= 1.
    The constructor synchronises `stream` (after the bounding box, and again at its end: everything the order holds is complete when
    it returns, so its methods may run on any stream) and keeps no reference to S.

    npoints, dimension, bits (31, 21; 64 in 1D), lo, hi (host tuples: the bounding box); perm, inverse (int64 device tensors, for
    torch indexing), keys (int64, ascending).

    Reorder the CLOUD (order.cloud, order.take for the fields) before building what must follow a moving cloud: an operator from
    order.operator has no geometry and no update()."""

    def __init__(self, S, stream=None):
        import torch
        dim = _cloud_dim(S)
        n = int(S.shape[0])
        if n < 1:
            raise ValueError("npoints must be >= 1")
        self._perm32 = torch.empty((n,), dtype=torch.int32, device=S.device)
        self._inverse32 = torch.empty((n,), dtype=torch.int32, device=S.device)
        self.keys = torch.empty((n,), dtype=torch.int64, device=S.device)
        box = (C.c_double * 6)()
        s, dev = _stream_and_device(S, stream)
        B.check(B.lib().wlsqm_hip_spatial_order_device(dim, n, _ptr(S), _ptr(self.keys), _ptr(self._perm32), _ptr(self._inverse32), box,
                                                       dev, s))
        with _torch_stream(stream, S.device):
            self.perm, self.inverse = self._perm32.long(), self._inverse32.long()
            # what the later calls read, on whatever stream they are given: made here, and complete when the constructor returns
            self._bad = torch.zeros((1,), dtype=torch.int32, device=S.device)
            self._minus = torch.full((n,), -1, dtype=torch.int32, device=S.device)
            torch.cuda.current_stream(S.device).synchronize()
        self.npoints, self.dimension, self.bits = n, dim, {1: 64, 2: 31, 3: 21}[dim]
        self.lo, self.hi = tuple(box[m] for m in range(dim)), tuple(box[3 + m] for m in range(dim))
        self._device = S.device

    def __repr__(self):
        return "SpatialOrder(npoints=%d, dimension=%d)" % (self.npoints, self.dimension)

    def keys_of(self, X, out=None, stream=None):
        """The keys (int64 device tensor, one per point) of other points X (n, dim) [1D: (n,)] under this order's box: where
        torch.searchsorted(order.keys, ...) places them.  Points outside the box clamp to its ends; a NaN coordinate gives the
        largest key.  Asynchronous; with `out` it allocates nothing and may be captured."""
        import torch
        if _cloud_dim(X) != self.dimension:
            raise ValueError("X must have %d coordinates per point, as the cloud of the order" % self.dimension)
        n = int(X.shape[0])
        if out is None:
            out = torch.empty((n,), dtype=torch.int64, device=X.device)
        else:
            _check(out, "out", "int64", 1)
            if int(out.shape[0]) != n or not out.is_contiguous():
                raise ValueError("out must be a contiguous int64 device tensor of shape (%d,)" % n)
        _same_device(X, out)
        lo, hi = (C.c_double * 3)(*self.lo), (C.c_double * 3)(*self.hi)
        s, dev = _stream_and_device(X, stream)
        B.check(B.lib().wlsqm_hip_spatial_keys_device(self.dimension, n, _ptr(X), lo, hi, _ptr(out), dev, s))
        return out

    def _along(self, t, dim, name):
        if not hasattr(t, "dim") or not hasattr(t, "index_select"):
            raise ValueError("argument %s must be a device (HIP) tensor" % name)
        if t.dim() < 1 or not -t.dim() <= int(dim) < t.dim() or int(t.shape[dim]) != self.npoints:
            raise ValueError("%s must have npoints = %d entries along dim %d; got shape %s" % (name, self.npoints, int(dim), tuple(t.shape)))
        if t.device != self._device:
            raise ValueError("all tensors must be on the same device")

    def take(self, t, dim=0, out=None):
        """t carried from the old order to the new one along `dim` (any dtype; npoints entries along dim): t.index_select(dim, perm)."""
        import torch
        self._along(t, dim, "t")
        return torch.index_select(t, int(dim), self.perm) if out is None else torch.index_select(t, int(dim), self.perm, out=out)

    def restore(self, t, dim=0, out=None):
        """The way back: t.index_select(dim, inverse), so that restore(take(t)) is t bit for bit."""
        import torch
        self._along(t, dim, "t")
        return torch.index_select(t, int(dim), self.inverse) if out is None else torch.index_select(t, int(dim), self.inverse, out=out)

    def _relabel(self, lists, nk, row_perm, own, check, out, stream, name):
        import torch
        ncases, K = int(lists.shape[0]), int(lists.shape[1])
        if nk is not None:
            _check(nk, "nk", "int32", 1)
            if nk.stride(0) != 1:
                raise ValueError("nk, knowns, weighting_method must have unit stride")
            _rows(ncases, nk=nk)
        if out is None:
            out = torch.empty((ncases, K), dtype=torch.int32, device=lists.device)
        else:
            _check(out, "out", "int32", 2)
            if tuple(out.shape) != (ncases, K) or not out.is_contiguous():
                raise ValueError("out must be a contiguous int32 device tensor of shape (%d, %d)" % (ncases, K))
            if _overlap(out, lists):
                raise ValueError("out must not overlap %s" % name)
        _same_device(self.perm, lists, nk, out)
        with _torch_stream(stream, self._device):
            if check:
                self._bad.zero_()
            s, dev = _stream_and_device(lists, stream)
            B.check(B.lib().wlsqm_hip_relabel_hoods_device(ncases, K, _ptr(lists), int(lists.stride(0)) if ncases > 1 else K, _ptr(nk),
                                                           _ptr(row_perm), _ptr(self._inverse32), self.npoints, _ptr(own), _ptr(out),
                                                           _ptr(self._bad) if check else None, dev, s))
            if check and int(self._bad.item()):
                raise ValueError("a live entry names a point outside 0 .. npoints - 1 = %d" % (self.npoints - 1))
        return out

    def hoods(self, hoods, nk=None, check=True, out=None, stream=None):
        """Neighbour lists in which case j is centred on point j — hoods (npoints, K) int32 with a contiguous last axis, nk (npoints,)
        int32 or None (every slot is live) — in the new order: out[i, k] = inverse[hoods[perm[i], k]] for k < nk[perm[i]], and the
        padding holds the row's own new number i, as ball pads its rows.  One kernel ("order-relabel").  The counts go with
        order.take(nk).  check=True reads one int back and raises ValueError when a live entry names no point; check=False reads
        nothing (such an entry becomes -1) and, with `out`, may be captured."""
        _check(hoods, "hoods", "int32", 2)
        if hoods.stride(1) != 1:
            raise ValueError("hoods must have a contiguous last axis")
        if int(hoods.shape[0]) != self.npoints:
            raise ValueError("hoods must have npoints = %d rows (case j centred on point j); got %d" % (self.npoints, int(hoods.shape[0])))
        return self._relabel(hoods, nk, self._perm32, None, check, out, stream, "hoods")

    def relabel(self, index, nk=None, check=True, out=None, stream=None):
        """An int32 device tensor of point numbers, (n,) or (n, K) with a contiguous last axis — a point_index, the lists of a subset of
        the cases — renumbered in place of its entries, rows unmoved: out = inverse[index].  With nk (n,) the slots k >= nk[j] of a 2D
        tensor are padding and become -1.  check as for hoods(); an index of more than npoints rows with nk allocates its padding in
        the call (every other form allocates nothing beside `out`)."""
        import torch
        if not hasattr(index, "dim") or index.dim() not in (1, 2):
            raise ValueError("index must be (n,) or (n, K)")
        _check(index, "index", "int32", index.dim())
        if index.stride(-1) != 1 and int(index.shape[-1]) > 1:
            raise ValueError("index must have a contiguous last axis")
        if index.dim() == 1:
            if nk is not None:
                raise ValueError("nk goes with a 2D index")
            if out is not None:
                _check(out, "out", "int32", 1)
                if tuple(out.shape) != tuple(index.shape) or not out.is_contiguous():
                    raise ValueError("out must be a contiguous int32 device tensor of shape (%d,)" % int(index.shape[0]))
            r = self._relabel(index.view(-1, 1), None, None, None, check, out.view(-1, 1) if out is not None else None, stream, "index")
            return out if out is not None else r.view(-1)
        own = None
        if nk is not None:
            own = self._minus
            if int(own.shape[0]) < int(index.shape[0]):                  # more rows than the cloud has points: the padding of this call
                with _torch_stream(stream, self._device):
                    own = torch.full((int(index.shape[0]),), -1, dtype=torch.int32, device=self._device)
        return self._relabel(index, nk, None, own, check, out, stream, "index")

    def cloud(self, S, hoods, nk, knowns, weighting_method, stream=None):
        """(S, hoods, nk, knowns, weighting_method) of an index-based cloud without point_index, all in the new order: what
        fit_cloud_device, StencilOperator and knn-built lists take.  take four times and hoods once."""
        with _torch_stream(stream, self._device):
            return (self.take(S).contiguous(), self.hoods(hoods, nk, stream=stream), self.take(nk), self.take(knowns),
                    self.take(weighting_method))

    def operator(self, op, stream=None):
        """P A P^T of a square StencilOperator whose row j names point j (ncases == npoints == order.npoints, no point_index;
        anything else raises ValueError), for every value plane: a new operator whose row i is the old row perm[i] with its columns
        renumbered.  The order of the entries inside a row is kept, so a row's sum has the same bits: op2.apply(order.take(F))
        restored is op.apply(F) bit for bit.  Built through op.coefficients(), the renumbered lists and
        StencilOperator.from_coefficients.  The transposed product sums a column's entries in case order, which the renumbering changes:
        op2.apply_transpose agrees with op's within the rounding of a sum in another order, not bit for bit.  An operator of a fit keeps
        its dimension, order and known_coef (rows carried to the new order), so op2.apply(order.take(F), known=order.take(known)) serves
        known derivatives as op.apply(F, known=known) does, bit for bit.  The result has no geometry and so no update(): reorder the
        cloud with order.cloud before building an operator that must follow a moving cloud."""
        import torch
        if not isinstance(op, StencilOperator):
            raise ValueError("op must be a StencilOperator")
        op._live()
        if op._point_index is not None or op.ncases != op.npoints or op.npoints != self.npoints:
            raise ValueError("order.operator takes a square operator whose row j names point j, of npoints = %d; got ncases = %d, "
                             "npoints = %d%s" % (self.npoints, op.ncases, op.npoints, ", with a point_index" if op._point_index is not None else ""))
        _same_device(self.perm, op._val)
        with _torch_stream(stream, self._device):
            slots, own = op.coefficients()
            live, dest, _ = op._slot_positions()
            lists = torch.zeros((op.ncases, op.K), dtype=torch.int32, device=self._device)
            lists[live] = op._m["col"][dest]
            nk = op._nk.to(torch.int32)
            mask = op._own_mask
            new = StencilOperator.from_coefficients(self.hoods(lists, nk, stream=stream), self.take(nk), self.take(slots, dim=1), op.npoints,
                                                    own=self.take(own, dim=1) if mask is not None else None,
                                                    own_mask=self.take(mask) if mask is not None else None, stream=stream)
            if op.known_coef is not None:
                # (ncases, no) per operator: what apply(known=) contracts with the known values of every case
                new.known_coef = self.take(op.known_coef, dim=1)
                new.has_known_derivatives = op.has_known_derivatives
            new.dimension, new.order, new.no = op.dimension, op.order, op.no
        return new


# ---- interpolation plans: search once, evaluate many times (csrc/interp_plan.hip) ----

def _diff_list(diff):
    """(list of int diffs, True when `diff` was a single int)."""
    if diff is None:
        raise ValueError("diff cannot be None")
    if hasattr(diff, "__len__") or hasattr(diff, "__iter__"):
        diffs = [int(d) for d in diff]
        if len(diffs) > 35:
            raise ValueError("at most 35 diffs per call; got %d" % len(diffs))
        return diffs, False
    return [int(diff)], True


class InterpolationPlan:
    """Everything about "these models evaluated at these points" that does not depend on the coefficients, computed once and
    kept on the device (wlsqm_hip_interp_plan_*): packed copies of the origins, the orders and the points, and per point the
    model (mode='nearest': the nearest origin, ties to the smaller index, or the caller's `I`) or the list of the models within
    `r` (mode='continuous').  ``evaluate()`` then only enqueues one kernel on a stream, so it can be captured into a graph
    behind the solve that makes the coefficients.

    xi (nmodels, dim) [1D: (nmodels,)] the origins, `order` an int or an int32 tensor (nmodels,), x (nx, dim) [1D: (nx,)] the
    evaluation points: float64 device tensors, contiguous last axis, any row stride.  I: int64 device tensor (nx,), nearest mode
    only; an entry outside 0 .. nmodels - 1 gives NaN at that point.  The constructor synchronises `stream`; the plan keeps no
    reference to its arguments (and never to a coefficient array)."""

    def __init__(self, xi, order, x, mode='nearest', r=None, I=None, stream=None):
        self._handle = None
        self._solver = None
        dim = self._check_args(None, x, mode, r, I)
        import torch
        if xi.dim() not in (1, 2) or (1 if xi.dim() == 1 else int(xi.shape[1])) != dim:
            raise ValueError("xi must be (nmodels,) or (nmodels, dim) with the coordinates of x; got %s" % (tuple(xi.shape),))
        _check(xi, "xi", "float64", xi.dim())
        self._geometry_requires_grad = self._geometry_requires_grad or bool(getattr(xi, "requires_grad", False))
        if xi.dim() == 2 and xi.stride(1) != 1:
            raise ValueError("Buffer and memoryview are not contiguous in the same dimension. (argument xi)")
        nmodels = int(xi.shape[0])
        if nmodels < 1:
            raise ValueError("xi must hold at least one origin")
        _same_device(x, xi, I)
        if hasattr(order, "data_ptr"):
            _check(order, "order", "int32", 1)
            _rows(nmodels, order=order)
            _same_device(x, order)
            order_t, order_stride = order, int(order.stride(0))
            self._max_no = _ndofs(dim, int(order[:nmodels].max())) if nmodels else 0
        else:
            self._max_no = _ndofs(dim, order)
            order_t, order_stride = torch.tensor([int(order)], dtype=torch.int32, device=x.device), 0
        s, dev = _stream_and_device(x, stream)
        h = C.c_void_p()
        B.check(B.lib().wlsqm_hip_interp_plan_create(C.byref(h), dev, s, dim, nmodels, _ptr(xi), int(xi.stride(0)), _ptr(order_t),
                                                     order_stride, self._mode_code, _ptr(x), int(x.stride(0)), int(x.shape[0]),
                                                     float(r) if r is not None else 0.0, _ptr(I)))
        self._finish(h, x, dim, nmodels)

    @classmethod
    def _for_solver(cls, solver, x, mode, r, I, stream):
        """ExpertSolver.interpolation_plan: the origins and orders are those of the solver's prepared geometry."""
        import weakref
        self = cls.__new__(cls)
        self._handle = None
        self._solver = None
        dim = self._check_args(solver.dimension, x, mode, r, I)
        _same_device(x, I)
        self._max_no = solver._max_no
        s, dev = _stream_and_device(x, stream)
        if dev != solver._device:
            raise ValueError("x is on device %d, the solver's geometry on device %d" % (dev, solver._device))
        h = C.c_void_p()
        B.check(B.lib().wlsqm_hip_interp_plan_create_expert(C.byref(h), solver._handle, s, self._mode_code, _ptr(x), int(x.stride(0)),
                                                            int(x.shape[0]), float(r) if r is not None else 0.0, _ptr(I)))
        self._finish(h, x, dim, solver.ncases)
        self._solver = weakref.ref(solver)
        return self

    def _check_args(self, dim, x, mode, r, I):
        if mode not in ('nearest', 'continuous'):
            raise ValueError("mode must be one of 'nearest', 'continuous'; got '%s'" % (mode,))
        if mode == 'continuous' and r is None:
            raise ValueError("r must be specified in mode='continuous'")
        if mode == 'continuous' and not float(r) > 0.0:
            raise ValueError("r must be positive; got %r" % (r,))
        if mode == 'continuous' and I is not None:
            raise ValueError("'I' names the model of every point in mode='nearest' only")
        if not hasattr(x, "data_ptr") or not hasattr(x, "is_cuda"):
            raise ValueError("argument x must be a device (HIP) tensor")
        if dim is None:
            dim = 1 if x.dim() == 1 else (int(x.shape[1]) if x.dim() == 2 else 0)
        if dim not in (1, 2, 3):
            raise ValueError("x must be (nx,) or (nx, dim) with dim 1..3; got %s" % (tuple(x.shape),))
        _check(x, "x", "float64", 1 if dim == 1 else 2)
        if dim > 1 and (int(x.shape[1]) != dim or (x.shape[0] > 0 and x.stride(1) != 1)):
            raise ValueError("x must be (nx, %d) with a contiguous last axis" % dim)
        if I is not None:
            _check(I, "I", "int64", 1)
            if I.shape[0] != x.shape[0]:
                raise ValueError("When 'I' is specified, 'I' must have the same length as x; got len(I) = %d, len(x) = %d."
                                 % (I.shape[0], x.shape[0]))
            if I.shape[0] > 1 and I.stride(0) != 1:
                raise ValueError("I must be contiguous")
        self._mode_code = 0 if mode == 'nearest' else 1
        self.mode, self.r = mode, (float(r) if mode == 'continuous' else None)
        self._geometry_requires_grad = bool(getattr(x, "requires_grad", False))      # differentiable_evaluate refuses such a plan
        return dim

    def _finish(self, h, x, dim, nmodels):
        self._handle = h
        self.dimension, self.nmodels, self.nx = dim, int(nmodels), int(x.shape[0])
        self._device = x.device
        self._I = None

    def close(self):
        """Release the device-side state now (also done by __del__); harmless when called again."""
        if getattr(self, "_handle", None):
            B.lib().wlsqm_hip_interp_plan_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _live(self):
        if not getattr(self, "_handle", None):
            raise RuntimeError("the interpolation plan has been closed")
        return self._handle

    def _result(self, single, ndiff, stacked, R, t=None):
        """(shape, field stride, diff stride) of what evaluate returns for an int diff (single) or ndiff of them, for one field or a
        stack of R: the strides are those of `t`, a tensor of that shape (0 for an axis the result does not have, and both 0 without
        a tensor or for one of another rank, which the caller rejects)."""
        shape = ((R,) if stacked else ()) + (() if single else (ndiff,)) + (self.nx,)
        if t is None or t.dim() != len(shape):
            return shape, 0, 0
        return shape, (int(t.stride(0)) if stacked else 0), (0 if single else int(t.stride(1 if stacked else 0)))

    def memory_used(self):
        """Bytes of device memory the plan holds."""
        b = C.c_int64(0)
        B.check(B.lib().wlsqm_hip_interp_plan_info(self._live(), None, None, None, C.byref(b)))
        return int(b.value)

    @property
    def I(self):
        """mode='nearest': the model of every point, an int64 device tensor (nx,) (what interpolate() returns as I); else None."""
        if self.mode != 'nearest':
            return None
        if self._I is None:
            import torch
            out = torch.empty((self.nx,), dtype=torch.int64, device=self._device)
            if self.nx > 0:
                B.check(B.lib().wlsqm_hip_interp_plan_export(self._live(), _stream_ptr(self._device, None), _ptr(out), None))
            self._I = out
        return self._I

    def lists(self):
        """mode='continuous': (off, idx), int64 device tensors (nx + 1,) and (number of entries,): the models within r of point m are
        idx[off[m]:off[m + 1]], in the order of the grid walk (cells in ascending (z, y, x), ascending model number inside a cell)."""
        if self.mode != 'continuous':
            raise ValueError("lists() belongs to mode='continuous'; a mode='nearest' plan has I")
        import torch
        n = C.c_int64(0)
        B.check(B.lib().wlsqm_hip_interp_plan_info(self._live(), None, C.byref(n), None, None))
        off = torch.empty((self.nx + 1,), dtype=torch.int64, device=self._device)
        idx = torch.empty((int(n.value),), dtype=torch.int64, device=self._device)
        B.check(B.lib().wlsqm_hip_interp_plan_export(self._handle, _stream_ptr(self._device, None), _ptr(off), _ptr(idx) if n.value else None))
        return off, idx

    def evaluate(self, diff=0, fi=None, out=None, stream=None):
        """Evaluate the models, or their derivatives `diff` (a DOF number, or a sequence of at most 35), at the plan's points.

        fi (nmodels, >= no) or a stack (R, nmodels, >= no): float64 device tensor(s) of coefficients, contiguous last axis;
        fi=None: the latest solve of the solver that made the plan.  Returns a device tensor (nx,) for an int `diff`,
        (ndiff, nx) for a sequence, with a leading axis R for a stack; `out` may be preallocated (that shape, contiguous last
        axis).  A diff the model does not have gives 0.  Every value is bit-identical whatever else the call asks for.
        Only enqueues one kernel on `stream` (default: torch's current stream): no allocation when `out` is given, no
        synchronisation.  Ordering against the solve that writes fi is stream order: evaluate on the stream of the solve."""
        import torch
        diffs, single = _diff_list(diff)
        h = self._live()
        ndiff = len(diffs)
        solver = None
        if fi is None:
            solver = self._solver() if self._solver is not None else None
            if solver is None or not getattr(solver, "_handle", None):
                raise RuntimeError("fi=None evaluates the latest solve of the solver that made the plan; this plan has none (any more)")
            R, stacked = 1, False
        else:
            _check(fi, "fi", "float64", fi.dim() if fi.dim() in (2, 3) else 2)
            if fi.device != self._device:
                raise ValueError("all tensors must be on the same device")
            stacked = fi.dim() == 3
            R = int(fi.shape[0]) if stacked else 1
            if fi.shape[-2] < self.nmodels or fi.shape[-1] < self._max_no or (fi.shape[-1] > 1 and fi.stride(-1) != 1):
                raise ValueError("fi must be (nmodels, >= no) = (%d, >= %d), or a stack of those, with a contiguous last axis; got %s"
                                 % (self.nmodels, self._max_no, tuple(fi.shape)))
        shape, so_f, so_d = self._result(single, ndiff, stacked, R, out)
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=self._device)
            _, so_f, so_d = self._result(single, ndiff, stacked, R, out)
        else:
            _check(out, "out", "float64", len(shape))
            if tuple(out.shape) != shape or out.device != self._device or (self.nx > 1 and out.stride(-1) != 1):
                raise ValueError("out must be a float64 device tensor of shape %s with a contiguous last axis" % (shape,))
        if self.nx == 0 or ndiff == 0 or R == 0:
            return out
        arr = (C.c_int32 * ndiff)(*diffs)
        s = _stream_ptr(self._device, stream)
        if fi is None:
            B.check(B.lib().wlsqm_hip_interp_plan_eval_expert(h, solver._handle, s, arr, ndiff, _ptr(out), so_d))
        else:
            B.check(B.lib().wlsqm_hip_interp_plan_eval_device(h, s, R, _ptr(fi), int(fi.stride(0)) if stacked else 0,
                                                              int(fi.stride(-2)), arr, ndiff, _ptr(out), so_f, so_d))
        return out

    # ---- the adjoint of evaluate (csrc/interp_plan.hip) ----

    def prepare_adjoint(self, stream=None):
        """Build the inverted index of the adjoint now (per model the points that use it, by a stable sort; continuous plans also
        keep the forward's weight sums): without this call the first evaluate_adjoint builds it — which allocates and synchronises,
        so it cannot happen inside a graph capture.  Synchronises `stream`.  Returns True when this call built the index (False: it
        was there already)."""
        h = self._live()
        had = self.adjoint_info()["built"]
        built = C.c_int(0)
        B.check(B.lib().wlsqm_hip_interp_plan_prepare_adjoint(h, _stream_ptr(self._device, stream), C.byref(built)))
        return bool(built.value) and not had

    def adjoint_info(self):
        """dict(built, nentries, max_len, nlong, threshold): whether the inverted index exists, its number of (model, point) entries,
        the longest list of a model, the number of models with more than `threshold` entries (they take the wave form of the adjoint
        kernel) — the three counts are None while the index is absent — and the threshold, a constant of the library."""
        n, longest, nlong, thr = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int32(0)
        B.check(B.lib().wlsqm_hip_interp_plan_adjoint_info(self._live(), C.byref(n), C.byref(longest), C.byref(nlong), C.byref(thr)))
        built = n.value >= 0
        return dict(built=built, nentries=int(n.value) if built else None, max_len=int(longest.value) if built else None,
                    nlong=int(nlong.value) if built else None, threshold=int(thr.value))

    def transposed_lists(self):
        """(toff, tpt), int64 device tensors (nmodels + 1,) and (number of entries,): the points that use model i are
        tpt[toff[i]:toff[i + 1]], in ascending point number.  Builds the index when it is absent (prepare_adjoint)."""
        import torch
        h = self._live()
        if not self.adjoint_info()["built"]:
            self.prepare_adjoint()
        n = self.adjoint_info()["nentries"]
        toff = torch.empty((self.nmodels + 1,), dtype=torch.int64, device=self._device)
        tpt = torch.empty((n,), dtype=torch.int64, device=self._device)
        B.check(B.lib().wlsqm_hip_interp_plan_export_transposed(h, _stream_ptr(self._device, None), _ptr(toff), _ptr(tpt) if n else None))
        return toff, tpt

    def evaluate_adjoint(self, g, diff=0, grad_fi=None, ncols=None, stream=None):
        """The adjoint of evaluate(diff, fi): from g = dL/d(evaluate's result) to grad_fi = dL/dfi.

        g has exactly the shape evaluate returns for that `diff` — (nx,) for an int, (ndiff, nx) for a sequence, with a leading axis
        R for a stack — float64 on the plan's device, contiguous last axis.  Returns grad_fi (nmodels, ncols) or (R, nmodels, ncols),
        ncols >= the plan's largest number of DOFs (the default); a preallocated grad_fi may have more rows and columns: exactly
        [:nmodels, :ncols] is written — every element of it, with exact zeros in the columns a model does not have and in the rows
        of models that no point uses — and nothing else.  g at a point whose value does not depend on fi (NaN in the forward) is
        never read; a diff given twice contributes twice.  No atomics: the bits of grad_fi of a field are a function of the plan and
        of that field's g (the same run to run, eager or replayed, alone or in a stack, with the diffs in any order).
        With the inverted index present (prepare_adjoint) the call only enqueues kernels on `stream`; without it the first call
        builds the index, which synchronises — RuntimeError when that would happen inside a graph capture."""
        import torch
        diffs, single = _diff_list(diff)
        ndiff = len(diffs)
        if not hasattr(g, "data_ptr") or not hasattr(g, "is_cuda"):
            raise ValueError("argument g must be a device (HIP) tensor")
        _check(g, "g", "float64", g.dim())
        h = self._live()
        base = 1 if single else 2
        if g.dim() not in (base, base + 1):
            raise ValueError("g must have the shape evaluate() returns for this diff: %s, or with a leading axis for a stack; got %s"
                             % (self._result(single, ndiff, False, 1)[0], tuple(g.shape)))
        stacked = g.dim() == base + 1
        R = int(g.shape[0]) if stacked else 1
        shape, sg_f, sg_d = self._result(single, ndiff, stacked, R, g)
        if tuple(g.shape) != shape or g.device != self._device or (self.nx > 1 and g.stride(-1) != 1):
            raise ValueError("g must be a float64 device tensor of shape %s with a contiguous last axis; got %s" % (shape, tuple(g.shape)))
        ncols = self._max_no if ncols is None else int(ncols)
        if ncols < self._max_no:
            raise ValueError("ncols = %d, need at least the plan's largest number of DOFs, %d" % (ncols, self._max_no))
        if grad_fi is None:
            grad_fi = torch.empty(((R,) if stacked else ()) + (self.nmodels, ncols), dtype=torch.float64, device=self._device)
        else:
            _check(grad_fi, "grad_fi", "float64", 3 if stacked else 2)
            if (grad_fi.device != self._device or (stacked and grad_fi.shape[0] != R) or grad_fi.shape[-2] < self.nmodels
                    or grad_fi.shape[-1] < ncols or (grad_fi.shape[-1] > 1 and grad_fi.stride(-1) != 1)):
                raise ValueError("grad_fi must be %s(>= %d, >= %d) on the plan's device with a contiguous last axis; got %s"
                                 % ("(%d, " % R if stacked else "", self.nmodels, ncols, tuple(grad_fi.shape)))
        if R == 0:
            return grad_fi
        arr = (C.c_int32 * max(ndiff, 1))(*diffs)
        B.check(B.lib().wlsqm_hip_interp_plan_eval_adjoint_device(h, _stream_ptr(self._device, stream), R, arr, ndiff, _ptr(g), sg_f, sg_d,
                                                                  _ptr(grad_fi), int(grad_fi.stride(0)) if stacked else 0,
                                                                  int(grad_fi.stride(-2)), ncols))
        return grad_fi


def differentiable_evaluate(plan, fi, diff=0, stream=None):
    """plan.evaluate(diff, fi) as a differentiable function of the coefficients fi (nmodels, >= no) or a stack (R, nmodels, >= no):
    the same bits as evaluate, with a grad_fn.  The backward pass is plan.evaluate_adjoint (one deterministic gather, no atomics),
    computed only when fi requires a gradient; dL/dfi has fi's full shape, zeros in the rows beyond nmodels and the columns beyond
    the plan's DOFs.  fi must be given: "the latest solve of the solver" is not a tensor autograd can see — chain it behind
    differentiable_solve.  The geometry (the x and xi the plan was made from) is not differentiable: ValueError when either
    required a gradient.  Call plan.prepare_adjoint() first when the backward pass is to be captured into a graph.
    Once differentiable."""
    if fi is None:
        raise ValueError("differentiable_evaluate needs the coefficients fi explicitly")
    _no_geometry_grad(plan)
    diffs, single = _diff_list(diff)
    return _autograd().Evaluate.apply(fi, plan, diffs[0] if single else diffs, stream)


# ---- stencil operators: differential operators of the fit as sparse matrices (csrc/stencil.hip) ----

def stencil_rows(dimension, order, *what, device=None):
    """The rows (lambda) of named operators for StencilOperator, in the DOF order of wlsqm.fitter.defs: a float64 tensor (nop, no) on
    `device` (None: the host; move it to the cloud's device).  Each `what` is 'value' (the fitted function value), 'gradient' (one row
    per axis), 'laplacian' (the sum of the pure second derivatives) or a DOF index such as wlsqm.i2_XY.  ValueError for a `what` that
    needs a higher order than `order`."""
    import torch
    from .fitter import defs
    dimension = int(dimension)
    no = _ndofs(dimension, order)
    axes = "XYZ"[:dimension]

    def row(*dofs):
        r = [0.0] * no
        for a in dofs:
            if isinstance(a, str):
                a = getattr(defs, "i%d_%s" % (dimension, a))
            if not 0 <= a < _NDOF[dimension][4]:
                raise ValueError("a %dD fit has the DOFs 0 .. %d; got %d" % (dimension, _NDOF[dimension][4] - 1, a))
            if a >= no:
                need = min(o for o in range(5) if _NDOF[dimension][o] > a)
                raise ValueError("DOF %d needs a fit of order %d or more; got order %d" % (a, need, int(order)))
            r[a] = 1.0
        return r

    rows = []
    for w in what:
        if w == "value":
            rows.append(row("F"))
        elif w == "gradient":
            rows.extend(row(a) for a in axes)
        elif w == "laplacian":
            rows.append(row(*(a + "2" for a in axes)))
        elif isinstance(w, int) and not isinstance(w, bool):
            rows.append(row(w))
        else:
            raise ValueError("what must be 'value', 'gradient', 'laplacian' or a DOF index; got %r" % (w,))
    if not rows:
        raise ValueError("stencil_rows needs at least one operator")
    return torch.tensor(rows, dtype=torch.float64, device=device)


def _torch_stream(stream, device):
    """The context in which torch operations run on the raw HIP stream `stream` (None / 0: torch's current stream)."""
    if not stream:
        return contextlib.nullcontext()
    import torch
    return torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=device))


def _extent(t):
    """[lo, hi) in bytes of the memory a strided tensor touches; None for an empty one."""
    lo = hi = 0
    for n, st in zip(t.shape, t.stride()):
        if n == 0:
            return None
        if st >= 0:
            hi += (n - 1) * st
        else:
            lo += (n - 1) * st
    size = t.element_size()
    return t.data_ptr() + lo * size, t.data_ptr() + (hi + 1) * size


def _overlap(a, b):
    ea, eb = _extent(a), _extent(b)
    return ea is not None and eb is not None and ea[0] < eb[1] and eb[0] < ea[1]


def _sell_pack(lens):
    """The SELL-64 frame of rows with `lens` (int64 device tensor, at least one row) live entries: (len int32, width int32, soff int64,
    total).  One host read."""
    import torch
    nrows = int(lens.shape[0])
    ns = (nrows + 63) // 64
    padded = torch.zeros((ns * 64,), dtype=torch.int64, device=lens.device)
    padded[:nrows] = lens
    width = padded.view(ns, 64).max(dim=1).values
    soff = torch.zeros((ns + 1,), dtype=torch.int64, device=lens.device)
    soff[1:] = torch.cumsum(64 * width, 0)
    return lens.to(torch.int32), width.to(torch.int32), soff, int(soff[-1])


def _sell_launch(m, nop, val_ptr, R, X_ptr, sx_f, sx_p, Y, sy_f, sy_o, sy_i, alpha, beta, dev, s):
    """One wlsqm_hip_sell_apply_device on the matrix m = dict(nrows, len, width, soff, col, total): the forward and the transposed product."""
    B.check(B.lib().wlsqm_hip_sell_apply_device(m["nrows"], int(m["width"].shape[0]), _ptr(m["len"]), _ptr(m["width"]), _ptr(m["soff"]),
                                                _ptr(m["col"]), C.c_void_p(val_ptr), m["total"], nop, R, C.c_void_p(X_ptr), sx_f, sx_p,
                                                _ptr(Y), sy_f, sy_o, sy_i, float(alpha), float(beta), dev, s))


class StencilOperator:
    """Differential operators of the fit as one sparse matrix on the device: row j holds the coefficients with which operator o,
    sum_a rows[o, a] d_a (a over the DOFs of wlsqm.fitter.defs), of the local model of case j depends on the point values, so that
    ``apply(F)[o, j]`` is what ``rows[o] . fi_out[j]`` is after ``fit_cloud_device`` on the same geometry — in one pass over
    4 + 8 nop bytes per neighbour, with no solve.  DESIGN.md section 16 has the algebra, the layout and the kernel.

    dimension, order (an int), S, hoods, nk, knowns, weighting_method, point_index: the geometry as fit_cloud_adjoint_device takes it.
    rows: float64 device tensor (nop, no), the same operators at every point, or (nop, ncases, no), variable coefficients (see
    stencil_rows).  The constructor runs fit_cloud_adjoint_device once per operator with g = rows[o] (the coefficients are that
    kernel's bits), packs them with torch operations on `stream` and synchronises; it keeps no reference to S.  3D orders 3 and 4 are
    not covered (ValueError, as the adjoint).

    The row of case j holds (hoods[j, k], slots[j, k]) for k < nk[j] in slot order, then, iff the function value is among the case's
    knowns (bit F), one entry (point_index[j], grad_fi[j, 0]): the dependence on the point's own value.  A column named twice in a
    row stays two entries.  Known DOFs other than F (and DOFs dropped by stray high mask bits, which leave the fit as they came) give an
    affine term: ``known_coef`` (nop, ncases, no) holds their coefficients (column 0 zeroed where it went into the matrix) and
    ``has_known_derivatives`` says whether any is non-zero; apply() then needs ``known``.

    Numerics: an F-known fit subtracts the point's own value before it sums; a stencil applies to F as given, and a derivative's
    coefficients sum to zero only to rounding.  A large constant offset in F costs digits in proportion to sum |c_k F_k|: subtract a
    reference value from F first."""

    def __init__(self, dimension, order, S, hoods, nk, knowns, weighting_method, rows, point_index=None, stream=None):
        import torch
        self._m = self._t = self._tval = self._tpair = None
        no = _adjoint_order(dimension, order)
        ncases, K = _cloud_geometry(dimension, S, hoods, nk, knowns, weighting_method, point_index,
                                    "S must be contiguous; hoods must have a contiguous last axis")
        if not hasattr(rows, "dim") or rows.dim() not in (2, 3):
            raise ValueError("rows must be (nop, no) or (nop, ncases, no)")
        per_case = rows.dim() == 3
        _double_rows(rows, "rows", ncases if per_case else 1, no, (int(dimension), int(order)), lead=1 if per_case else 0)
        nop = int(rows.shape[0])
        if nop < 1:
            raise ValueError(_FEW_ROWS % ("rows", nop, 1))
        _same_device(S, hoods, nk, knowns, weighting_method, point_index, rows)
        npoints, device = int(S.shape[0]), S.device
        z = lambda *shape: torch.empty(shape, dtype=torch.float64, device=device)
        with _torch_stream(stream, device):
            slots, gfi, scratch = z(nop, ncases, K), z(nop, ncases, no), z(npoints)
        for o in range(nop):
            with _torch_stream(stream, device):
                g = rows[o] if per_case else rows[o, :no].expand(ncases, no).contiguous()
            fit_cloud_adjoint_device(dimension, order, S, hoods, nk, knowns, weighting_method, g, point_index=point_index,
                                     grad_F=scratch, grad_fi=gfi[o], stream=stream, slots=slots[o])
        with _torch_stream(stream, device):
            fknown = (knowns[:ncases] & 1) != 0
            zero = torch.zeros((), dtype=torch.float64, device=device)
            own = torch.where(fknown[None, :], gfi[:, :, 0], zero)
            gfi[:, :, 0] = torch.where(fknown[None, :], zero, gfi[:, :, 0])
            pts = point_index[:ncases].long() if point_index is not None else torch.arange(ncases, device=device)
            self._pack(hoods[:ncases], nk[:ncases], slots, own, fknown, pts, npoints)
            self.known_coef = gfi
            # what update() answers from the masks alone: some DOF other than an F that went into the matrix is known or dropped
            full = (1 << no) - 1
            low = knowns[:ncases] & full
            structural = ((low & ~1) != 0) | (((knowns[:ncases] & ~full) != 0) & (low != full))
            self.has_known_derivatives, self._structural = torch.stack([(gfi != 0).any(), structural.any()]).tolist()
        self.dimension, self.order, self.no = int(dimension), int(order), no
        self._geo, self._rows = (hoods, nk, knowns, weighting_method, point_index), rows
        self._point_index = point_index

    @classmethod
    def from_coefficients(cls, hoods, nk, slots, npoints, own=None, own_mask=None, point_index=None, stream=None):
        """The operator of given coefficients (no fit): row j holds (hoods[j, k], slots[o, j, k]) for k < nk[j], then, where own_mask[j],
        (point_index[j], own[o, j]).  hoods (ncases, K) int32, nk (ncases,) int32, slots (nop, ncases, K) and own (nop, ncases) float64,
        own_mask (ncases,) bool, point_index (ncases,) int32 (default: row j names point j): device tensors.  Only live slots are
        looked at: the padding of hoods and slots may hold anything.  Synchronises."""
        import torch
        self = cls.__new__(cls)
        self._m = self._t = self._tval = self._tpair = None
        _check(hoods, "hoods", "int32", 2); _check(nk, "nk", "int32", 1)
        ncases, K = int(hoods.shape[0]), int(hoods.shape[1])
        _rows(ncases, nk=nk)
        _double_rows(slots, "slots", ncases, K, lead=1,
                     says="slots must be at least (nop, ncases, %d) with a contiguous last axis; got %s" % (K, tuple(slots.shape)))
        nop = int(slots.shape[0])
        if nop < 1 or ncases < 1:
            raise ValueError(_FEW_ROWS % ("slots", min(nop, ncases), 1))
        if (own is None) != (own_mask is None):
            raise ValueError("own and own_mask go together")
        if own is not None:
            _double_rows(own, "own", nop, ncases, says="own must be at least (%d, %d) with a contiguous last axis; got %s"
                         % (nop, ncases, tuple(own.shape)))
            _check(own_mask, "own_mask", "bool", 1)
            _rows(ncases, own_mask=own_mask)
        if point_index is not None:
            _check(point_index, "point_index", "int32", 1)
            _rows(ncases, point_index=point_index)
        _same_device(hoods, nk, slots, own, own_mask, point_index)
        device = hoods.device
        with _torch_stream(stream, device):
            pts = point_index[:ncases].long() if point_index is not None else torch.arange(ncases, device=device)
            self._pack(hoods, nk[:ncases], slots[:, :ncases, :K], own[:nop, :ncases] if own is not None else None,
                       own_mask[:ncases] if own_mask is not None else None, pts, int(npoints))
        self.known_coef, self.has_known_derivatives = None, False
        self._geo = self._rows = None
        self._point_index = point_index
        self.dimension = self.order = None
        self.no = 0
        return self

    def _pack(self, hoods, nk, slots, own, own_mask, pts, npoints):
        """The SELL-64 arrays from per-slot coefficients (torch operations on the current stream; three host reads)."""
        import torch
        nop, ncases, K = (int(v) for v in slots.shape)
        device = hoods.device
        nkc = nk.long().clamp(0, K)
        lens = nkc + own_mask.long() if own_mask is not None else nkc
        len32, width, soff, total = _sell_pack(lens)
        j = torch.arange(ncases, device=device)
        live = torch.arange(K, device=device)[None, :] < nkc[:, None]
        base = soff[j // 64] + j % 64
        dest = (base[:, None] + 64 * torch.arange(K, device=device)[None, :])[live]
        cols = hoods[live].long()
        bad = ((cols < 0) | (cols >= npoints)).any()
        col = torch.zeros((total,), dtype=torch.int32, device=device)
        val = torch.zeros((nop, total), dtype=torch.float64, device=device)
        col[dest] = cols.to(torch.int32)
        val[:, dest] = slots[:, live]
        if own_mask is not None:
            d_own = (base + 64 * nkc)[own_mask]
            c_own = pts[own_mask]
            bad = bad | ((c_own < 0) | (c_own >= npoints)).any()
            col[d_own] = c_own.to(torch.int32)
            val[:, d_own] = own[:, own_mask]
        if bool(bad):
            raise ValueError("a live entry names a point outside 0 .. npoints - 1 = %d" % (npoints - 1))
        self._m = dict(nrows=ncases, len=len32, width=width, soff=soff, col=col, total=total)
        self._val, self._nk, self._own_mask = val, nkc, own_mask
        self._nnz = int(lens.sum())
        self.nop, self.ncases, self.npoints, self.K, self._device = nop, ncases, int(npoints), K, device

    def _live(self):
        if getattr(self, "_m", None) is None:
            raise RuntimeError("the stencil operator has been closed")
        return self._m

    def close(self):
        """Release the device memory now; harmless when called again."""
        self._m = self._t = self._val = self._tval = self._tpair = self._nk = self._own_mask = self.known_coef = None
        self._geo = self._rows = self._point_index = None

    def memory_used(self):
        """Bytes of device memory the operator holds (the transposed matrix included once built, with the index pair that update()
        refreshes its values through).  The caller's hoods, nk, knowns, weighting_method, point_index and rows, which the operator
        references for update(), are not counted."""
        self._live()
        held = list(self._m.values()) + [self._val, self._nk, self._own_mask, self.known_coef]
        if self._t is not None:
            held += list(self._t.values()) + [self._tval, getattr(self, "_tpair", None)]
        return sum(t.numel() * t.element_size() for t in held if hasattr(t, "numel"))

    def update(self, S, hoods=None, rows=None, check=True, stream=None):
        """Recompute every value plane, the own entries and known_coef for the points where they are now, S (>= npoints rows, as the
        constructor takes it), into the arrays the operator already holds: the constructor's coefficients on the new geometry (its
        bits for the systems up to 10 unknowns), by one fused kernel (csrc/fit_adjoint.hip, "stencil-build": one factorisation per case
        for all operators).  The operator keeps references to the hoods, nk, knowns, weighting_method, point_index and rows it was
        built with (not to S) and reads them here: the caller must not resize or free them.

        rows: new operators, the same nop and the same (nop, no) or (nop, ncases, no) form.  hoods: new neighbour lists of the same
        shape and dtype for the same nk (a fixed-k search redone); the columns are rewritten and a transposed matrix built for the old
        ones is dropped (fill_transposed is None again, the next transposed use rebuilds it).  Without new hoods a built transposed
        matrix has its values refreshed by a second kernel.  Changing nk or knowns needs a new operator.

        check=True verifies that every live index is in 0 .. npoints - 1 before anything is enqueued (torch operations, one host read;
        ValueError as the constructor's; RuntimeError inside a graph capture).  check=False enqueues kernels only: no allocation, no
        synchronisation, at most two launches on `stream`, so update + apply can be captured and replayed after S.copy_(...).
        Afterwards has_known_derivatives is structural: true iff some case has a known or dropped DOF other than an F that went into
        the matrix, whatever the values of rows (the constructor's answer looks at the coefficients, and may be False where this is
        True).  RuntimeError for an operator from from_coefficients (no fit to redo) or a closed one."""
        m = self._live()
        if getattr(self, "_geo", None) is None:
            raise RuntimeError("the stencil operator was made from coefficients: there is no fit to redo")
        old_hoods, nk, knowns, weighting_method, point_index = self._geo
        new_hoods = old_hoods if hoods is None else hoods
        if not hasattr(S, "dim") or not hasattr(S, "is_cuda"):
            raise ValueError("argument S must be a device (HIP) tensor")
        if hoods is not None:
            _check(hoods, "hoods", "int32", 2)
            if tuple(hoods.shape) != (self.ncases, self.K):
                raise ValueError("hoods must be (%d, %d) int32 as the operator was built with; got %s: another shape needs a new operator"
                                 % (self.ncases, self.K, tuple(hoods.shape)))
        ncases, K = _cloud_geometry(self.dimension, S, new_hoods, nk, knowns, weighting_method, point_index,
                                    "S must be contiguous; hoods must have a contiguous last axis")
        if S.shape[0] < self.npoints:
            raise ValueError("S has fewer points than the operator's npoints = %d" % self.npoints)
        new_rows = self._rows if rows is None else rows
        per_case = self._rows.dim() == 3
        if rows is not None:
            if not hasattr(rows, "dim") or rows.dim() != self._rows.dim() or rows.shape[0] != self.nop:
                raise ValueError("rows must keep the operator's form, %s with nop = %d"
                                 % ("(nop, ncases, no)" if per_case else "(nop, no)", self.nop))
            _double_rows(rows, "rows", ncases if per_case else 1, self.no, (self.dimension, self.order), lead=1 if per_case else 0)
        _same_device(self._val, S, new_hoods, new_rows)
        s, dev = _stream_and_device(S, stream)
        if check:
            import torch
            with _torch_stream(stream, self._device):
                if self._device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("update checks the indices with a host read and the stream is capturing: pass check=False inside the capture")
                live = torch.arange(K, device=self._device)[None, :] < self._nk[:, None]
                cols = new_hoods[:ncases][live]
                bad = ((cols < 0) | (cols >= self.npoints)).any()
                if self._own_mask is not None:
                    pts = point_index[:ncases][self._own_mask] if point_index is not None else None
                    if pts is not None:
                        bad = bad | ((pts < 0) | (pts >= self.npoints)).any()
                if bool(bad):
                    raise ValueError("a live entry names a point outside 0 .. npoints - 1 = %d" % (self.npoints - 1))
        B.check(B.lib().wlsqm_hip_stencil_build_device(
            self.dimension, self.order, ncases, K, _ptr(S), _ptr(new_hoods), int(new_hoods.stride(0)), _ptr(point_index), _ptr(nk),
            _ptr(knowns), _ptr(weighting_method), _ptr(new_rows), int(new_rows.stride(0)), int(new_rows.stride(1)) if per_case else 0,
            self.nop, _ptr(m["len"]), _ptr(m["soff"]), _ptr(m["col"]) if hoods is not None else None, _ptr(self._val), m["total"],
            _ptr(self.known_coef), int(self.known_coef.stride(0)), int(self.known_coef.stride(1)), dev, s))
        tpair = getattr(self, "_tpair", None)
        if hoods is not None or tpair is None:
            self._t = self._tval = self._tpair = None       # built for other columns (or too large for the pair): rebuilt at the next use
        elif self._t is not None:
            B.check(B.lib().wlsqm_hip_sell_permute_device(int(tpair.shape[1]), _ptr(tpair[0]), _ptr(tpair[1]),
                                                          _ptr(self._val), m["total"], _ptr(self._tval), self._t["total"], self.nop, dev, s))
        self._geo, self._rows = (new_hoods, nk, knowns, weighting_method, point_index), new_rows
        self.has_known_derivatives = self._structural
        return self

    @property
    def fill(self):
        """Live entries over stored entries of the forward matrix (1.0: no padding)."""
        m = self._live()
        return self._nnz / m["total"] if m["total"] else 1.0

    @property
    def fill_transposed(self):
        """The same for the transposed matrix; None until prepare_transpose has built it."""
        self._live()
        if self._t is None:
            return None
        return self._nnz / self._t["total"] if self._t["total"] else 1.0

    def _entries(self):
        """(src, row): the position in col / val and the row of every live entry, in (case, entry) order."""
        import torch
        m = self._live()
        device = self._device
        j = torch.arange(self.ncases, device=device)
        e = torch.arange(self.K + 1, device=device)
        live = e[None, :] < m["len"].long()[:, None]
        base = m["soff"][j // 64] + j % 64
        return (base[:, None] + 64 * e[None, :])[live], j[:, None].expand(self.ncases, self.K + 1)[live]

    def _apply_args(self, F, known):
        """The checks of apply's inputs: (stacked, R)."""
        self._live()
        if not hasattr(F, "dim") or not hasattr(F, "is_cuda"):
            raise ValueError("argument F must be a device (HIP) tensor")
        stacked = F.dim() == 2
        _check(F, "F", "float64", 2 if stacked else 1)
        R = int(F.shape[0]) if stacked else 1
        if F.shape[-1] < self.npoints:
            raise ValueError("F has fewer entries than S has points")
        if R < 1:
            raise ValueError(_FEW_ROWS % ("F", R, 1))
        if F.device != self._device:
            raise ValueError("all tensors must be on the same device")
        if known is None:
            if self.has_known_derivatives:
                raise ValueError("the operator depends on known DOFs other than F: pass known=, (ncases, >= %d) with the known values of "
                                 "every case in their DOF columns (the fi that the fit would be given), or a stack of those" % self.no)
        elif self.known_coef is not None:
            lead = 1 if hasattr(known, "dim") and known.dim() == 3 else 0
            _double_rows(known, "known", self.ncases, self.no, lead=lead)
            if lead and (not stacked or known.shape[0] != R):
                raise ValueError("known is a stack of %d, F %s" % (known.shape[0], "a stack of %d" % R if stacked else "one field"))
            _same_device(F, known)
        return stacked, R

    def _out(self, out, shape, beta, against, device):
        import torch
        if out is None:
            return (torch.zeros if beta != 0 else torch.empty)(shape, dtype=torch.float64, device=device)
        _check(out, "out", "float64", len(shape))
        if tuple(out.shape) != tuple(shape):
            raise ValueError("out must be a float64 device tensor of shape %s; got %s" % (tuple(shape), tuple(out.shape)))
        if out.device != device:
            raise ValueError("all tensors must be on the same device")
        if _overlap(out, against):
            raise ValueError("out overlaps the input in memory: the product does not run in place")
        return out

    def apply(self, F, out=None, alpha=1.0, beta=0.0, known=None, stream=None):
        """out = alpha * (A F + the known term) + beta * out.  F (npoints,) or (R, npoints), float64 on the operator's device, any
        strides; returns (nop, ncases) or (R, nop, ncases) (`out`: that shape, any strides, not overlapping F; beta == 0 never reads
        it).  known: (ncases, >= no) or a stack (R, ncases, >= no), the known values in their DOF columns; required (ValueError) when
        has_known_derivatives, its term is added by torch operations on the same stream.  Otherwise one kernel launch on `stream`
        (default: torch's current stream): no allocation when `out` is given, no synchronisation, so it can be captured."""
        import torch
        stacked, R = self._apply_args(F, known)
        m = self._m
        out = self._out(out, ((R,) if stacked else ()) + (self.nop, self.ncases), beta, F, self._device)
        s, dev = _stream_and_device(F, stream)
        _sell_launch(m, self.nop, self._val.data_ptr(), R, F.data_ptr(), int(F.stride(0)) if stacked else 0, int(F.stride(-1)), out,
                     int(out.stride(0)) if stacked else 0, int(out.stride(-2)), int(out.stride(-1)), alpha, beta, dev, s)
        if known is not None and self.has_known_derivatives:
            with _torch_stream(stream, self._device):
                out.add_(torch.einsum("oja,...ja->...oj", self.known_coef, known[..., :self.ncases, :self.no]), alpha=float(alpha))
        return out

    def _known_adjoint(self, g, known_shape, stream):
        """dL/dknown from g = dL/d(apply's result): known_coef-weighted, zeros where the forward reads nothing."""
        import torch
        with _torch_stream(stream, self._device):
            out = torch.zeros(known_shape, dtype=torch.float64, device=self._device)
            if self.known_coef is not None:
                if g.dim() == 3 and len(known_shape) == 2:
                    g = g.sum(dim=0)
                out[..., :self.ncases, :self.no] = torch.einsum("...oj,oja->...ja", g, self.known_coef)
        return out

    def prepare_transpose(self, stream=None):
        """Build the transposed matrix now, npoints x ncases in the same format: a stable sort of the entries by column, ties in
        (case, entry) order, so the transposed sums are deterministic.  Without this call the first transposed use builds it, which
        allocates and synchronises — RuntimeError when that would happen inside a graph capture.  Returns True when this call built it."""
        import torch
        m = self._live()
        if self._t is not None:
            return False
        with _torch_stream(stream, self._device):
            if self._device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the operator has no transposed matrix yet and the stream is capturing: call prepare_transpose before the capture")
            src, row = self._entries()
            c = m["col"][src].long()
            c_sorted, order = torch.sort(c, stable=True)
            tlens = torch.bincount(c, minlength=self.npoints)
            start = torch.cumsum(tlens, 0) - tlens
            et = torch.arange(c.shape[0], device=self._device) - start[c_sorted]
            len32, width, soff, total = _sell_pack(tlens)
            dest = soff[c_sorted // 64] + 64 * et + c_sorted % 64
            tcol = torch.zeros((total,), dtype=torch.int32, device=self._device)
            tval = torch.zeros((self.nop, total), dtype=torch.float64, device=self._device)
            tcol[dest] = row[order].to(torch.int32)
            tval[:, dest] = self._val[:, src[order]]
            self._t = dict(nrows=self.npoints, len=len32, width=width, soff=soff, col=tcol, total=total)
            self._tval = tval
            # (dest, src) of every live entry, for update(): one 8-byte pair per entry; positions beyond int32 go without (update then
            # drops the transposed matrix and the next use rebuilds it)
            self._tpair = torch.stack([dest, src[order]]).to(torch.int32) if max(total, m["total"]) < 2 ** 31 else None
        return True

    def apply_transpose(self, g, out=None, alpha=1.0, beta=0.0, stream=None):
        """out = alpha * sum_o A_o^T g[o] + beta * out.  g (nop, ncases) or (R, nop, ncases), any strides; returns (npoints,) or
        (R, npoints).  The same kernel on the transposed matrix, one launch per operator (each adds to `out` in operator order): no
        atomics, the bits are a function of the operator and of g.  Builds the transposed matrix at the first use (prepare_transpose)."""
        self._live()
        if not hasattr(g, "dim") or not hasattr(g, "is_cuda"):
            raise ValueError("argument g must be a device (HIP) tensor")
        stacked = g.dim() == 3
        _check(g, "g", "float64", 3 if stacked else 2)
        if tuple(g.shape[-2:]) != (self.nop, self.ncases):
            raise ValueError("g must be (nop, ncases) = (%d, %d), or a stack of those; got %s" % (self.nop, self.ncases, tuple(g.shape)))
        R = int(g.shape[0]) if stacked else 1
        if R < 1:
            raise ValueError(_FEW_ROWS % ("g", R, 1))
        if g.device != self._device:
            raise ValueError("all tensors must be on the same device")
        out = self._out(out, ((R,) if stacked else ()) + (self.npoints,), beta, g, self._device)
        if self._t is None:
            self.prepare_transpose(stream)
        s, dev = _stream_and_device(g, stream)
        for o in range(self.nop):
            _sell_launch(self._t, 1, self._tval.data_ptr() + 8 * o * self._t["total"], R, g.data_ptr() + 8 * o * int(g.stride(-2)),
                         int(g.stride(0)) if stacked else 0, int(g.stride(-1)), out, int(out.stride(0)) if stacked else 0, 0,
                         int(out.stride(-1)), alpha, beta if o == 0 else 1.0, dev, s)
        return out

    def _slot_positions(self):
        """(live (ncases, K) bool, dest: the position in col / val of every live neighbour slot, d_own: that of every own entry or None)."""
        import torch
        m = self._live()
        device = self._device
        j = torch.arange(self.ncases, device=device)
        k = torch.arange(self.K, device=device)
        live = k[None, :] < self._nk[:, None]
        base = m["soff"][j // 64] + j % 64
        dest = (base[:, None] + 64 * k[None, :])[live]
        return live, dest, (base + 64 * self._nk)[self._own_mask] if self._own_mask is not None else None

    def _unpack(self, planes):
        import torch
        nop = int(planes.shape[0])
        slots = torch.zeros((nop, self.ncases, self.K), dtype=torch.float64, device=self._device)
        own = torch.zeros((nop, self.ncases), dtype=torch.float64, device=self._device)
        live, dest, d_own = self._slot_positions()
        slots[:, live] = planes[:, dest]
        if d_own is not None:
            own[:, self._own_mask] = planes[:, d_own]
        return slots, own

    def coefficients(self):
        """(slots (nop, ncases, K), own (nop, ncases)): the coefficients unpacked, per neighbour slot and on the point's own value;
        exact zeros in the padding and where a row has no own entry."""
        self._live()
        return self._unpack(self._val)

    def unpack(self, plane):
        """(slots (ncases, K), own (ncases,)) of any plane in the operator's layout, a contiguous float64 device tensor (total,) — a
        value plane, or StencilSolver.gradients' `values`: what coefficients() does for the operator's own planes, exact zeros in the
        padding and where a row has no own entry.  Torch operations on the current stream."""
        m = self._live()
        if not hasattr(plane, "dim") or not hasattr(plane, "is_cuda"):
            raise ValueError("argument plane must be a device (HIP) tensor")
        _check(plane, "plane", "float64", 1)
        if tuple(plane.shape) != (m["total"],) or (m["total"] > 1 and plane.stride(0) != 1):
            raise ValueError("plane must be a contiguous float64 device tensor of shape (%d,), the operator's layout; got shape %s with "
                             "strides %s" % (m["total"], tuple(plane.shape), tuple(plane.stride())))
        if plane.device != self._device:
            raise ValueError("all tensors must be on the same device")
        slots, own = self._unpack(plane.view(1, -1))
        return slots[0], own[0]

    def set_coefficients(self, slots, own=None, stream=None):
        """Write new coefficients into the arrays the operator holds: slots (nop, ncases, K) and, for an operator with own entries, own
        (nop, ncases), as from_coefficients takes them (only live slots and rows with an own entry are looked at).  The structure stays
        and the padding is untouched.  A built transposed matrix has its values refreshed as update() does (dropped where it is too
        large for the index pair; the next transposed use rebuilds it).  Torch index operations on `stream` and at most one kernel
        launch; no host read.  ValueError when `own` is given to an operator without own entries or missing for one with them."""
        m = self._live()
        for t, name in ((slots, "slots"), (own, "own")):
            if t is not None and (not hasattr(t, "dim") or not hasattr(t, "is_cuda")):
                raise ValueError("argument %s must be a device (HIP) tensor" % name)
        _double_rows(slots, "slots", self.ncases, self.K, lead=1,
                     says="slots must be at least (nop, ncases, %d) with a contiguous last axis; got %s" % (self.K, tuple(slots.shape)))
        if int(slots.shape[0]) != self.nop:
            raise ValueError("slots has %d value planes, the operator %d" % (int(slots.shape[0]), self.nop))
        if (own is None) != (self._own_mask is None):
            raise ValueError("own goes together with an operator that has own entries: this one has %s"
                             % ("none" if self._own_mask is None else "them"))
        if own is not None:
            _double_rows(own, "own", self.nop, self.ncases, says="own must be at least (%d, %d) with a contiguous last axis; got %s"
                         % (self.nop, self.ncases, tuple(own.shape)))
        _same_device(self._val, slots, own)
        with _torch_stream(stream, self._device):
            live, dest, d_own = self._slot_positions()
            self._val[:, dest] = slots.detach()[:, :self.ncases, :self.K][:, live]
            if d_own is not None:
                self._val[:, d_own] = own.detach()[:self.nop, :self.ncases][:, self._own_mask]
        tpair = getattr(self, "_tpair", None)
        if tpair is None:
            self._t = self._tval = None                     # too large for the pair: rebuilt at the next use
        elif self._t is not None:
            s, dev = _stream_and_device(self._val, stream)
            B.check(B.lib().wlsqm_hip_sell_permute_device(int(tpair.shape[1]), _ptr(tpair[0]), _ptr(tpair[1]),
                                                          _ptr(self._val), m["total"], _ptr(self._tval), self._t["total"], self.nop, dev, s))
        return self

    def to_sparse_csr(self, o=0):
        """Operator `o` as a torch.sparse_csr_tensor (ncases, npoints): columns sorted, duplicates summed."""
        import torch
        self._live()
        if not 0 <= int(o) < self.nop:
            raise ValueError("the operator has %d value planes; got o = %d" % (self.nop, int(o)))
        src, row = self._entries()
        coo = torch.sparse_coo_tensor(torch.stack([row, self._m["col"][src].long()]), self._val[int(o), src],
                                      (self.ncases, self.npoints))
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)       # torch announces its CSR support as beta at the first use
            return coo.coalesce().to_sparse_csr()


def differentiable_stencil_apply(op, F, known=None, stream=None):
    """op.apply(F, known=known) as a differentiable function of F (npoints,) or (R, npoints) and of `known`: the same bits as apply,
    with a grad_fn.  The backward pass is op.apply_transpose (the same kernel on the transposed matrix, no atomics), computed only
    when F requires a gradient; dL/dF has F's full shape, zeros beyond the operator's points.  `known` receives the
    known_coef-weighted gradients.  Call op.prepare_transpose() first when the backward pass is to be captured into a graph.
    The backward pass reads the operator as it is then: an op.update between forward and backward invalidates the graph, as any
    in-place change of a saved tensor does (it is not detected).  Once differentiable."""
    op._apply_args(F, known)                       # before anything is detached
    return _autograd().StencilApply.apply(F, known, op, stream)


SolveGradients = collections.namedtuple("SolveGradients", "values diag scale")
SolveGradients.__doc__ = """What StencilSolver.gradients returns: dL/d(the entries of the value plane) in the operator's layout, dL/d(diag)
and dL/d(scale) (a 0-d device tensor); None for what was not asked for."""

SystemGradients = collections.namedtuple("SystemGradients", "values diag")
SystemGradients.__doc__ = """What StencilSystemSolver.gradients returns: dL/d(the entries of every value plane), (nop, total) in the operator's
layout, and dL/d(diag), (m, m, npoints); None for what was not asked for."""

SolveInfo = collections.namedtuple("SolveInfo", "status iterations residual")
SolveInfo.__doc__ = """What a StencilSolver says of a solve.  status: 0 converged, 1 iteration limit, 2 breakdown (rho = 0 or (r0, v) = 0),
3 a non-finite scalar, 4 a zero or non-finite Jacobi diagonal, a singular or non-finite block of a BlockJacobi or of an OverlappingBlocks or a singular row of an ApproximateInverse, -1 still running (enqueue with fewer iterations than the solve needs
always ends in 1).  With method="bicgstab2", 2 is rho0 = 0, (rt, u1) = 0 or (rt, u2) = 0.  iterations: those completed.  residual: the recursive ||r||_2 (NaN with status 4: no residual was formed)."""


class BlockJacobi:
    """The block-Jacobi preconditioner of a StencilSolver: P = blockdiag(M_BB)^-1, the exact inverses of the
    diagonal blocks of `block` consecutive rows (8, 16 or 32), the last block cut at npoints.  It pays where consecutive rows are
    neighbours in space — a cloud in Morton order (wlsqm.hip.SpatialOrder), as every large workload of this project is; on a cloud in
    random order the blocks hold next to nothing off their diagonals and it does no better than "jacobi".
    refresh=True: P is recomputed from the operator's arrays at the start of every solve / enqueue, as the Jacobi diagonal is.
    refresh=False: P is computed at the first start and again only by solver.refresh() — for time loops on a fixed operator."""

    def __init__(self, block=16, refresh=True):
        if isinstance(block, bool) or block not in (8, 16, 32):
            raise ValueError("block must be 8, 16 or 32; got %r" % (block,))
        self.block, self.refresh = int(block), bool(refresh)

    def __repr__(self):
        return "BlockJacobi(block=%d, refresh=%r)" % (self.block, self.refresh)


class ApproximateInverse:
    """The sparse approximate inverse preconditioner of a StencilSolver: P = Q, the matrix on M's own pattern whose
    row i minimises ||q^T M - e_i^T||_2, so that Q M ~ I: one small dense least-squares problem per row ("krylov-spai"), applied as one
    more sparse product on the operator's structure.  Unlike the blocks it couples every row with all its neighbours, whatever the
    order of the cloud: for the large steps (tau ~ 1, above all in 3D) that neither "jacobi" nor a BlockJacobi reaches.  An iteration
    costs about twice a Jacobi iteration.  Rows of up to 64 neighbours (and their own entry); one right-hand side (nfields = 1); both methods.
    refresh: what it means for a BlockJacobi: True recomputes Q at the start of every solve / enqueue, False computes it at the first
    start and again only by solver.refresh()."""

    def __init__(self, refresh=True):
        self.refresh = bool(refresh)

    def __repr__(self):
        return "ApproximateInverse(refresh=%r)" % (self.refresh,)


class OverlappingBlocks:
    """The overlapping-block (restricted additive Schwarz) preconditioner of a StencilSolver.  Block B, `block`
    consecutive rows (8, 16 or 32), is extended by the rows that its equations name most often, up to `rows` rows in all (32 or 64, more
    than block); the extended block of M is inverted exactly ("krylov-schwarz-build") and only the block's own rows of the inverse are
    kept, so P v is a gather and a small dense product per row ("krylov-schwarz-apply"), without a scatter.  It couples the blocks, which
    is what a BlockJacobi lacks on the large steps (tau ~ 1, above all in 3D): on I - h^2 Lap_h in 3D at 2000 points the reference takes
    a tenth of BlockJacobi(16)'s iterations under BiCGSTAB(2), and plain BiCGSTAB converges where it breaks down with the blocks.  It is
    a one-level method: the count still grows with the cloud.  Like a BlockJacobi it wants a cloud in Morton order.
    The sets depend on the operator's structure alone and are found once, when the solver is made; op.update never invalidates them.
    An iteration is 10 launches (19 per cycle of "bicgstab2") and reads 8 rows bytes of the plane per row and application.  One
    right-hand side (nfields = 1); both methods.
    refresh: what it means for a BlockJacobi: True recomputes P at the start of every solve / enqueue, False computes it at the first
    start and again only by solver.refresh()."""

    def __init__(self, block=32, rows=64, refresh=True):
        if isinstance(block, bool) or block not in (8, 16, 32):
            raise ValueError("block must be 8, 16 or 32; got %r" % (block,))
        if isinstance(rows, bool) or rows not in (32, 64) or rows <= block:
            raise ValueError("rows must be 32 or 64, and more than block (%d); got %r" % (block, rows))
        self.block, self.rows, self.refresh = int(block), int(rows), bool(refresh)

    def __repr__(self):
        return "OverlappingBlocks(block=%d, rows=%d, refresh=%r)" % (self.block, self.rows, self.refresh)


def overlapping_sets(m, block, rows):
    """The index table of an OverlappingBlocks on the SELL-64 arrays `m` of a square operator: int32 (nblocks, rows) on their device.
    Row B: the block's own rows s .. e - 1 (e = min(s + block, n)), then the rows - (e - s) columns outside s .. e - 1 that the stored
    entries of those rows name most often (duplicates counted, ties to the smaller index) in ascending order, then -1.  tests/
    _krylov_schwarz_ref.py states it in numpy.  torch operations on the structure alone; one host read (the longest row)."""
    import torch
    n, dev = int(m["nrows"]), m["len"].device
    nblocks = (n + block - 1) // block
    table = torch.full((nblocks, rows), -1, dtype=torch.int64, device=dev)
    own = torch.arange(nblocks * block, device=dev).view(nblocks, block)
    table[:, :block] = torch.where(own < n, own, torch.full_like(own, -1))
    lens = torch.minimum(m["len"].long(), m["width"].long().repeat_interleave(64)[:n])
    most = int(lens.max()) if n else 0
    e = torch.arange(most, device=dev)
    step = max(block, (1 << 18) // block * block)                       # rows per pass: bounds the temporaries at 10^6 points and beyond
    for lo in range(0, n, step):
        j = torch.arange(lo, min(n, lo + step), device=dev)
        live = e[None, :] < lens[j][:, None]
        src = ((m["soff"][j // 64] + j % 64)[:, None] + 64 * e[None, :])[live]
        blk = (j // block)[:, None].expand(-1, most)[live]
        col = m["col"][src].long()
        outside = (col < blk * block) | (col >= blk * block + block)
        key, count = torch.unique(blk[outside] * n + col[outside], return_counts=True)         # ascending in (block, column)
        kb = key // n
        order = torch.sort(-count, stable=True)[1]                       # the largest count first, the smaller column at a tie
        order = order[torch.sort(kb[order], stable=True)[1]]             # ... within each block
        kb, key = kb[order], key[order]
        at = torch.arange(kb.shape[0], device=dev)
        head = torch.full((nblocks,), kb.shape[0], dtype=torch.int64, device=dev).scatter_reduce(0, kb, at, "amin")
        room = rows - torch.clamp(n - torch.arange(nblocks, device=dev) * block, max=block)
        keep = at - head[kb] < room[kb]
        key = torch.sort(key[keep])[0]                                   # the chosen ones in ascending order, block by block
        kb = key // n
        at = torch.arange(kb.shape[0], device=dev)
        head = torch.full((nblocks,), kb.shape[0], dtype=torch.int64, device=dev).scatter_reduce(0, kb, at, "amin")
        table[kb, (rows - room[kb]) + at - head[kb]] = key - kb * n
    return table.to(torch.int32).contiguous()


class PointBlockJacobi:
    """The block-Jacobi preconditioner of a StencilSystemSolver: P = blockdiag(M_BB)^-1, the exact inverses of
    the diagonal blocks of `points` consecutive points with all m unknowns of each — m points consecutive rows of the flat (npoints, m)
    vectors, the last block cut at npoints.  points counts points, not rows: 1 <= points and m points <= 32; None takes the largest
    value with m points <= 16 (16 / 8 / 5 / 4 points for m = 1 / 2 / 3 / 4); points=1 is the m x m point-block diagonal.
    It pays where consecutive points are neighbours in space — a cloud in Morton order (wlsqm.hip.SpatialOrder) — and the more the
    larger the cloud: on 2D elasticity at 1000 points the reference takes 84 iterations with 16 points per block where "jacobi" takes
    213.  In 3D ten points are a small cluster and the blocks gain little (39 against 40 at 1000 points).  DESIGN.md section 27 has
    the counts, which tests/test_krylov_system_block_host.py holds, and what was measured at 10^6 points: an iteration costs 1.08 to
    1.38 of Jacobi's (what the plane's bytes predict), the factor one to seven iterations at every start (refresh=False: once), and
    on the Dirichlet elasticity systems the time to solution gained a tenth at best in 2D and lost in 3D.  The plane is
    8 NB^2 / R bytes per row.
    refresh: what it means for a BlockJacobi: True recomputes P at the start of every solve / enqueue, False computes it at the first
    start and again only by solver.refresh()."""

    def __init__(self, points=None, refresh=True):
        if points is not None and (isinstance(points, bool) or not isinstance(points, int) or points < 1):
            raise ValueError("points must be None or an int >= 1, the points of a block; got %r" % (points,))
        self.points, self.refresh = points, bool(refresh)

    def __repr__(self):
        return "PointBlockJacobi(points=%r, refresh=%r)" % (self.points, self.refresh)


class StencilSolver:
    """Solves M x = b with M = diag(d) + scale * A_o, A_o value plane `o` of a square StencilOperator, by BiCGSTAB resident on the
    device (csrc/krylov.hip): eight kernel launches per iteration, two passes over the matrix, every dot product
    formed in the pass that produces its vector, no host synchronisation inside `enqueue`.  The bits of x, of the iteration count and
    of the residual are a function of the operator, diag, scale, b, x and the tolerances: no atomics, eager and captured runs agree.

    op: square — ncases == npoints, row j the equation of point j (point_index None or the identity; checked here with one host read,
    ValueError) — not closed, and without known derivatives (their affine term belongs in b).  The solver reads the operator's arrays
    at every solve: after op.update(...) it solves with the new values, and nothing has to be called on the solver.
    diag: a float, or a contiguous float64 device tensor (npoints,) that is read at every solve (the caller may change it in place).
    preconditioner: "jacobi" (the inverse of M's diagonal, recomputed at the start of every solve), None, or a BlockJacobi (the
    inverses of the diagonal blocks of 8, 16 or 32 consecutive rows: for large steps on a cloud in Morton order, which
    wlsqm.hip.SpatialOrder produces for a cloud, its lists or a finished operator).
    All workspace, 9 npoints + 2 ceil(npoints / 256) + 16 doubles, is allocated here; close() releases it.  A BlockJacobi adds its
    plane, 64 block ceil(npoints / 64) + ceil(npoints / 256) doubles, and a second one for M^T at the first transposed use
    (prepare_transpose).
    solve, enqueue and product take transpose=True for M^T; gradients() and differentiable_stencil_solve carry a loss through the
    solve.
    nfields (1 .. 8): how many right-hand sides solve_many, enqueue_many and product_many take at once, as
    independent solves that share every pass over the matrix.  nfields=1 allocates and runs exactly what a solver without it does;
    above that the workspace holds 8 vectors at the pitch 2, 4 or 8 (the next one above nfields) and a head per field
    (wlsqm_hip_krylov_many_workspace_bytes), and solve, enqueue and product still serve single vectors.
    method: "bicgstab" (the default: everything above), or "bicgstab2" for the large steps on which BiCGSTAB breaks down or wanders
    (tau >= 1, above all in 3D, with a BlockJacobi on a cloud in Morton order): BiCGSTAB(2) of Sleijpen and Fokkema, two BiCG steps and
    then one residual minimisation over two dimensions.  Every method of the solver serves it, with every
    preconditioner, transposed solves and differentiable_stencil_solve included; nfields must be 1.  A cycle is 4 products in 14
    launches and counts as 2 iterations, so `iterations`, `maxiter` and `check_every` mean what they mean for "bicgstab"; the stop is
    taken at the end of a cycle, so a solve may pass an odd maxiter by one, and enqueue(iterations=k) enqueues ceil(k / 2) cycles.
    Status 2 is then rho0 = 0, (rt, u1) = 0 or (rt, u2) = 0.  The workspace is 10 npoints + 5 ceil(npoints / 256) + 16 doubles.
    preconditioner=ApproximateInverse(): the sparse approximate inverse Q on the matrix's own pattern, with
    either method: 10 launches per iteration, 19 per cycle (Q is applied by launches of its own).  It adds its planes, npoints +
    ceil(npoints / 64) + the operator's stored entries doubles, and those of Q^T (the same numbers moved into the transposed
    structure) at the first transposed use.  refresh(), precondition(v) and preconditioner_matrix() serve it; a row whose least-squares
    problem is singular is status 4.  Rows of more than 64 neighbours and nfields > 1 are refused here (ValueError).
    preconditioner=OverlappingBlocks(block, rows): blocks extended by the rows they name most often, inverted exactly, their own rows
    kept, with either method: 10 launches per iteration, 19 per cycle.  It adds its index table, 4 rows
    ceil(npoints / block) bytes, found here from the operator's structure, its plane, 64 rows ceil(npoints / 64) + (64 / block)
    ceil(npoints / 64) doubles, and a second plane for M^T at the first transposed use.  refresh(), precondition(v) and
    preconditioner_overlapping_blocks() serve it; an extended block that cannot be inverted is status 4.  nfields > 1 is refused."""

    def __init__(self, op, o=0, diag=1.0, scale=1.0, preconditioner="jacobi", nfields=1, method="bicgstab"):
        self._ws = None
        if isinstance(nfields, bool) or not isinstance(nfields, int) or not 1 <= nfields <= 8:
            raise ValueError("nfields must be an int, 1 .. 8; got %r" % (nfields,))
        self.nfields = nfields
        if method not in ("bicgstab", "bicgstab2"):
            raise ValueError("method must be 'bicgstab' or 'bicgstab2'; got %r" % (method,))
        if method == "bicgstab2" and nfields > 1:
            raise ValueError("method 'bicgstab2' solves one right-hand side at a time: nfields must be 1; got %d" % nfields)
        self.method, self._l2 = method, method == "bicgstab2"
        if not isinstance(op, StencilOperator):
            raise ValueError("op must be a StencilOperator")
        op._live()
        if op.ncases != op.npoints:
            raise ValueError("the operator must be square: it has %d rows (cases) for %d points" % (op.ncases, op.npoints))
        if op.has_known_derivatives:
            raise ValueError("the operator depends on known DOFs other than F: their affine term belongs in b, build the operator without them")
        if not 0 <= int(o) < op.nop:
            raise ValueError("the operator has %d value planes; got o = %d" % (op.nop, int(o)))
        self._block = preconditioner if isinstance(preconditioner, BlockJacobi) else None
        self._spai = preconditioner if isinstance(preconditioner, ApproximateInverse) else None
        self._schwarz = preconditioner if isinstance(preconditioner, OverlappingBlocks) else None
        self._table = None
        if isinstance(preconditioner, PointBlockJacobi):
            raise ValueError("a PointBlockJacobi belongs to a StencilSystemSolver, whose blocks count points of m unknowns; a StencilSolver "
                             "takes a BlockJacobi, whose block counts rows")
        if self._block is None and self._spai is None and self._schwarz is None and preconditioner not in ("jacobi", None):
            raise ValueError("preconditioner must be 'jacobi' or None, or a BlockJacobi, an ApproximateInverse or an OverlappingBlocks; "
                             "got %r" % (preconditioner,))
        if self._spai is not None and nfields > 1:
            raise ValueError("an ApproximateInverse preconditions one right-hand side at a time: nfields must be 1; got %d" % nfields)
        if self._schwarz is not None and nfields > 1:
            raise ValueError("an OverlappingBlocks preconditions one right-hand side at a time: nfields must be 1; got %d" % nfields)
        self._planes = self._planes_t = self._planes_t_of = None
        self._factored = self._factored_t = False
        self._op, self._o, self._jacobi = op, int(o), 1 if preconditioner == "jacobi" else 0
        self.npoints, self._device = op.npoints, op._device
        self.scale = float(scale)
        if hasattr(diag, "dim"):
            self._vector(diag, "diag")
            self.diag = diag
        else:
            self.diag = float(diag)
        import torch
        pi = getattr(op, "_point_index", None)
        if pi is not None and not bool((pi[:op.ncases].long() == torch.arange(op.ncases, device=pi.device)).all()):
            raise ValueError("row j of the operator must be the equation of point j: point_index must be None or the identity")
        if self._spai is not None:                                      # one host read: the widest slice and the longest row
            self._max_width, most = torch.stack([op._m["width"].max().long(), op._nk.max().long()]).tolist()
            if most > 64:                                               # the own entry of an F-known row may come on top: 65 stored entries
                raise ValueError("an ApproximateInverse serves rows of up to 64 neighbours; the operator's longest row has %d" % most)
        if self._l2:
            nbytes = int(B.lib().wlsqm_hip_krylov_l2_workspace_bytes(self.npoints))
        elif nfields == 1:
            nbytes = int(B.lib().wlsqm_hip_krylov_workspace_bytes(self.npoints))
        else:
            nbytes = int(B.lib().wlsqm_hip_krylov_many_workspace_bytes(self.npoints, nfields))
        self._ws = torch.zeros((nbytes // 8,), dtype=torch.float64, device=self._device)
        if self._schwarz is not None:                                   # the sets: from the structure alone, once
            self._table = overlapping_sets(op._m, self._schwarz.block, self._schwarz.rows)
        if self._block is not None or self._spai is not None or self._schwarz is not None:
            self._planes = self._new_planes()

    def _new_planes(self, transpose=False):
        import torch
        if self._spai is not None:
            nbytes = int(B.lib().wlsqm_hip_krylov_spai_bytes(self.npoints, (self._op._t if transpose else self._op._m)["total"]))
        elif self._schwarz is not None:
            nbytes = int(B.lib().wlsqm_hip_krylov_schwarz_bytes(self.npoints, self._schwarz.block, self._schwarz.rows))
        else:
            nbytes = int(B.lib().wlsqm_hip_krylov_block_bytes(self.npoints, self._block.block))
        return torch.zeros((nbytes // 8,), dtype=torch.float64, device=self._device)

    def _live(self):
        if getattr(self, "_ws", None) is None:
            raise RuntimeError("the stencil solver has been closed")
        return self._op._live()

    def close(self):
        """Release the workspace now; harmless when called again.  The operator stays the caller's."""
        self._ws = self._op = self._planes = self._planes_t = self._planes_t_of = self._table = None
        if hasattr(self.__dict__.get("diag"), "dim"):
            self.diag = None

    def memory_used(self):
        """Bytes of device memory the solver holds (the operator's and a diag tensor are the caller's)."""
        self._live()
        return sum(t.numel() * t.element_size() for t in (self._ws, self._planes, self._planes_t, self._table) if t is not None)

    def _vector(self, t, name):
        if not hasattr(t, "dim") or not hasattr(t, "is_cuda"):
            raise ValueError("argument %s must be a device (HIP) tensor" % name)
        _check(t, name, "float64", 1)
        if tuple(t.shape) != (self.npoints,) or (self.npoints > 1 and t.stride(0) != 1):
            raise ValueError("%s must be a contiguous float64 device tensor of shape (%d,); got shape %s with strides %s"
                             % (name, self.npoints, tuple(t.shape), tuple(t.stride())))
        if t.device != self._device:
            raise ValueError("all tensors must be on the same device")

    def _vectors(self, **named):
        """The checks of the vectors of a call: each one (npoints,) float64 contiguous on the operator's device, none overlapping
        another, the diag tensor or the workspace."""
        self._live()
        for name, t in named.items():
            self._vector(t, name)
        self._disjoint(named)

    def _disjoint(self, named):
        """ValueError when one of the tensors `named` overlaps another of them, the diag tensor, the workspace or a block plane."""
        held = dict(named, workspace=self._ws)
        if hasattr(self.diag, "dim"):
            held["diag"] = self.diag
        for name, t in (("the preconditioner's blocks", self._planes), ("the preconditioner's transposed blocks", self._planes_t)):
            if t is not None:
                held[name] = t
        names = list(held)
        for i, a in enumerate(names):
            for b in names[i + 1:]:
                if a in named and _overlap(held[a], held[b]):
                    raise ValueError("%s overlaps %s in memory" % (a, b))

    @staticmethod
    def _tolerances(rtol, atol, maxiter):
        rtol, atol, maxiter = float(rtol), float(atol), int(maxiter)
        if not (0.0 <= rtol < float("inf")) or not (0.0 <= atol < float("inf")):
            raise ValueError("rtol and atol must be finite and >= 0; got %r, %r" % (rtol, atol))
        if not 0 <= maxiter < 2 ** 31:
            raise ValueError("the number of iterations must be 0 .. 2^31 - 1; got %d" % maxiter)
        return rtol, atol, maxiter

    def _system(self, transpose=False):
        """The system's arguments of the C entry points: M, or M^T = diag(d) + scale * A_o^T on the operator's transposed arrays."""
        m, val = (self._op._t, self._op._tval) if transpose else (self._op._m, self._op._val)
        d = self.diag
        return (m["nrows"], int(m["width"].shape[0]), _ptr(m["len"]), _ptr(m["width"]), _ptr(m["soff"]), _ptr(m["col"]),
                C.c_void_p(val.data_ptr() + 8 * self._o * m["total"]), _ptr(d) if hasattr(d, "dim") else None,
                0.0 if hasattr(d, "dim") else d, self.scale)

    def _transposed(self, transpose, stream):
        """The operator's transposed matrix, and a BlockJacobi's or an OverlappingBlocks' transposed plane, built at the first transposed use (prepare_transpose:
        RuntimeError inside a capture)."""
        if transpose and (self._op._t is None or (self._dense_blocks() and self._planes_t is None) or self._stale_transposed()):
            self.prepare_transpose(stream)
        return bool(transpose)

    def _dense_blocks(self):
        """A BlockJacobi or an OverlappingBlocks: the transposed plane has the forward one's size and the factor's launch fills both."""
        return self._block is not None or self._schwarz is not None

    def _stale_transposed(self):
        """An ApproximateInverse's transposed planes are missing, or belong to a transposed matrix that the operator has dropped."""
        return self._spai is not None and (self._planes_t is None or self._planes_t_of is not self._op._tpair)

    def prepare_transpose(self, stream=None):
        """Build now what a transposed solve needs: the operator's transposed matrix (op.prepare_transpose) and, with a BlockJacobi or an
        OverlappingBlocks, the plane of the transposed inverse blocks (an ApproximateInverse: the planes of Q^T).  Without this call the first transposed use builds them, which allocates — RuntimeError
        when that would happen inside a graph capture.  The plane is filled by the next factor: at the next transposed start, from the
        operator as it is then (also with refresh=False), and from then on together with the forward plane.  Returns True when this
        call built something."""
        import torch
        self._live()
        built = False
        if self._op._t is None:
            built = self._op.prepare_transpose(stream)
        if self._dense_blocks() and self._planes_t is None:
            with _torch_stream(stream, self._device):
                if self._device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("the solver has no transposed preconditioner blocks yet and the stream is capturing: call "
                                       "prepare_transpose before the capture")
                self._planes_t = self._new_planes()
            self._factored_t = False
            built = True
        if self._stale_transposed():
            if self._op._tpair is None:
                raise ValueError("the operator's transposed matrix is too large for its index pairs (2^31 stored entries): an "
                                 "ApproximateInverse cannot carry its values into it")
            with _torch_stream(stream, self._device):
                if self._device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("the solver has no transposed approximate inverse yet and the stream is capturing: call "
                                       "prepare_transpose before the capture")
                self._planes_t = self._new_planes(transpose=True)
            self._planes_t_of = self._op._tpair
            self._factored_t = False
            built = True
        return built

    def _block_args(self, transpose=False):
        return self._block.block, _ptr(self._planes_t if transpose else self._planes)

    def _factor(self, dev, s, transpose=False, force=False):
        """"krylov-blocks" ("krylov-spai", "krylov-schwarz-build") when P is due: at every start with refresh=True, else at the first one, when the transposed plane is new, and
        from refresh().  One launch on the forward matrix, which fills the transposed plane too when this start needs it or, with
        refresh=False, whenever it exists (the two stay the inverses of the same blocks)."""
        bj = self._block if self._block is not None else self._spai if self._spai is not None else self._schwarz
        if not (force or bj.refresh or not self._factored or (transpose and not self._factored_t)):
            return
        both = self._planes_t is not None and (transpose or not bj.refresh or force)
        if self._spai is not None:          # "krylov-spai": Q from the forward matrix, and its values moved into the transposed planes
            both = both and not self._stale_transposed()
            pair = self._op._tpair if both else None
            B.check(B.lib().wlsqm_hip_krylov_spai_build_device(*self._system(False), self._max_width, _ptr(self._planes),
                                                               int(pair.shape[1]) if both else 0, _ptr(pair[0]) if both else None,
                                                               _ptr(pair[1]) if both else None, _ptr(self._planes_t) if both else None,
                                                               dev, s))
        elif self._schwarz is not None:     # "krylov-schwarz-build": the kept rows of the inverses of M's and of M^T's extended blocks
            B.check(B.lib().wlsqm_hip_krylov_schwarz_build_device(*self._system(False), *self._schwarz_args(),
                                                                  _ptr(self._planes_t) if both else None, dev, s))
        else:
            B.check(B.lib().wlsqm_hip_krylov_block_factor_device(*self._system(False), bj.block, _ptr(self._planes),
                                                                 _ptr(self._planes_t) if both else None, dev, s))
        self._factored = True
        if both:
            self._factored_t = True
        elif bj.refresh:
            self._factored_t = False

    def refresh(self, stream=None):
        """Recompute a BlockJacobi's, an ApproximateInverse's or an OverlappingBlocks' P from the operator's arrays as they are on `stream` now: what
        refresh=False leaves to the caller (after op.update, set_coefficients or a change of diag or scale).  One kernel launch (two
        with an ApproximateInverse's transposed planes), no allocation, no host read: capturable."""
        self._live()
        if self._planes is None:
            raise ValueError("refresh() belongs to a BlockJacobi preconditioner, an ApproximateInverse or an OverlappingBlocks; this "
                             "solver's is %s, which every solve recomputes"
                             % ("'jacobi'" if self._jacobi else "None"))
        s, dev = _stream_and_device(self._planes, stream)
        self._factor(dev, s, force=True)
        return self

    def precondition(self, v, out=None, stream=None, transpose=False):
        """z = P v (P^T v with transpose=True), P the BlockJacobi's block inverses as the next solve would use them: factored first when
        due (refresh=True: always).  One launch ("krylov-precondition") behind the factor's; v and out (npoints,) float64 contiguous,
        not overlapping.  With an ApproximateInverse: z = Q v ("krylov-spai-apply"), Q^T v on the transposed structure.  With an
        OverlappingBlocks: the kept rows applied to the gathered v ("krylov-schwarz-apply" behind "krylov-schwarz-build"); transpose=True
        applies the second plane, the same preconditioner of M^T, which is not P^T.  ValueError on a solver with none of them."""
        import torch
        self._live()
        if self._planes is None:
            raise ValueError("precondition() belongs to a BlockJacobi preconditioner, an ApproximateInverse or an OverlappingBlocks")
        if out is None:
            with _torch_stream(stream, self._device):
                out = torch.empty((self.npoints,), dtype=torch.float64, device=self._device)
        self._vectors(v=v, out=out)
        transpose = self._transposed(transpose, stream)
        s, dev = _stream_and_device(v, stream)
        self._factor(dev, s, transpose)
        if self._spai is not None:                                       # "krylov-spai-apply": out = Q v, or Q^T v on the transposed structure
            B.check(B.lib().wlsqm_hip_krylov_spai_apply_device(*self._system(transpose)[:6], *self._spai_args(transpose)[1:], _ptr(v),
                                                               _ptr(out), dev, s))
            return out
        if self._schwarz is not None:                                    # "krylov-schwarz-apply": the kept rows on M's sets, or on M^T's
            B.check(B.lib().wlsqm_hip_krylov_schwarz_apply_device(self.npoints, *self._schwarz_args(transpose), _ptr(v), _ptr(out), dev, s))
            return out
        B.check(B.lib().wlsqm_hip_krylov_block_precondition_device(self.npoints, *self._block_args(transpose), _ptr(v), _ptr(out), dev, s))
        return out

    def preconditioner_blocks(self, stream=None):
        """The inverse blocks as a new tensor (nblocks, block, block), nblocks = ceil(npoints / block), factored first when due; the
        padding of the last block is the identity.  It allocates the result, so it is not for a graph capture."""
        self._live()
        if self._block is None:
            raise ValueError("preconditioner_blocks() belongs to a BlockJacobi preconditioner")
        nb = self._block.block
        s, dev = _stream_and_device(self._planes, stream)
        self._factor(dev, s)
        nslices = (self.npoints + 63) // 64
        with _torch_stream(stream, self._device):
            W = self._planes[:nslices * nb * 64].view(nslices, nb, 64 // nb, nb)          # [slice, j, block of the slice, i]
            return W.permute(0, 2, 3, 1).reshape(-1, nb, nb)[:(self.npoints + nb - 1) // nb].clone()

    def _schwarz_args(self, transpose=False):
        return self._schwarz.block, self._schwarz.rows, _ptr(self._table), _ptr(self._planes_t if transpose else self._planes)

    def preconditioner_overlapping_blocks(self, transpose=False, stream=None):
        """(table, W) of an OverlappingBlocks: the index table, int32 (nblocks, rows), -1 where a set is shorter, and the kept rows of
        the inverses as a new tensor (nblocks, block, rows), W[B, i, q] the weight of v[table[B, q]] in z[B block + i]; built first
        when due.  transpose=True: the plane that a transposed solve applies, the kept rows of the inverses of the transposed extended
        blocks.  The rows of the last block beyond npoints are zeros, and so is every column at a -1.  It allocates the result: not
        for a graph capture."""
        self._live()
        if self._schwarz is None:
            raise ValueError("preconditioner_overlapping_blocks() belongs to an OverlappingBlocks preconditioner")
        transpose = self._transposed(transpose, stream)
        nb, rows = self._schwarz.block, self._schwarz.rows
        s, dev = _stream_and_device(self._planes, stream)
        self._factor(dev, s, transpose)
        nslices = (self.npoints + 63) // 64
        with _torch_stream(stream, self._device):
            W = (self._planes_t if transpose else self._planes)[:nslices * rows * 64].view(nslices, rows, 64 // nb, nb)   # [slice, q, block, i]
            return self._table.clone(), W.permute(0, 2, 3, 1).reshape(-1, nb, rows)[:(self.npoints + nb - 1) // nb].clone()

    def _spai_args(self, transpose=False):
        return int(self._l2), _ptr(self._planes_t if transpose else self._planes)

    def _spai_parts(self, transpose=False):
        """(m, qd, qv): the structure that Q (or Q^T) lies on, its diagonal and its plane as views of the solver's planes."""
        n = self.npoints
        planes = self._planes_t if transpose else self._planes
        return (self._op._t if transpose else self._op._m), planes[:n], planes[n + (n + 63) // 64:]

    def preconditioner_matrix(self, transpose=False, stream=None):
        """An ApproximateInverse's Q (Q^T with transpose=True, from the planes that a transposed solve applies) as a new
        torch.sparse_csr_tensor (npoints, npoints), built first when due (refresh=True: always).  The entries are coalesced: a dead
        slot — one whose column an earlier slot of its row names, coefficient exactly 0.0 — is dropped into the live one of its
        column; preconditioner_coefficients() shows them apart.  It allocates and reads on the host: not for a graph capture."""
        import torch
        self._live()
        if self._spai is None:
            raise ValueError("preconditioner_matrix() belongs to an ApproximateInverse preconditioner")
        self._no_capture("preconditioner_matrix", stream)
        transpose = self._transposed(transpose, stream)
        s, dev = _stream_and_device(self._planes, stream)
        self._factor(dev, s, transpose)
        m, qd, qv = self._spai_parts(transpose)
        n = self.npoints
        with _torch_stream(stream, self._device):
            lens = m["len"].long()
            j, e = torch.arange(n, device=self._device), torch.arange(int(lens.max()), device=self._device)
            live = e[None, :] < lens[:, None]
            src = ((m["soff"][j // 64] + j % 64)[:, None] + 64 * e[None, :])[live]
            rows = torch.cat([j, j[:, None].expand(n, e.shape[0])[live]])
            cols = torch.cat([j, m["col"][src].long()])
            coo = torch.sparse_coo_tensor(torch.stack([rows, cols]), torch.cat([qd, qv[src]]), (n, n))
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", UserWarning)
                return coo.coalesce().to_sparse_csr()

    def preconditioner_coefficients(self, stream=None):
        """(qd (npoints,), slots (npoints, K), own (npoints,)): an ApproximateInverse's Q slot by slot, as the operator's
        coefficients() lays a value plane out: built first when due; exact zeros in the dead slots and in the padding."""
        self._live()
        if self._spai is None:
            raise ValueError("preconditioner_coefficients() belongs to an ApproximateInverse preconditioner")
        self._no_capture("preconditioner_coefficients", stream)
        s, dev = _stream_and_device(self._planes, stream)
        self._factor(dev, s)
        m, qd, qv = self._spai_parts()
        with _torch_stream(stream, self._device):
            slots, own = self._op.unpack(qv)
            return qd.clone(), slots, own

    def _no_capture(self, what, stream):
        import torch
        with _torch_stream(stream, self._device):
            if self._device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("%s reads the solve's scalars on the host and the stream is capturing: use enqueue inside the capture "
                                   "and info() after the replay" % what)

    def _precond_args(self, transpose=False):
        """(precond, planes) of the entry points that take every preconditioner: 0 none, 1 Jacobi, or the block size and its plane."""
        if self._block is not None:
            return self._block_args(transpose)
        return self._jacobi, None

    def _start(self, b, x, rtol, atol, maxiter, dev, s, transpose=False):
        if self._planes is not None:
            self._factor(dev, s, transpose)
        if self._schwarz is not None:
            B.check(B.lib().wlsqm_hip_krylov_schwarz_start_device(*self._system(transpose), int(self._l2), *self._schwarz_args(transpose),
                                                                  _ptr(b), _ptr(x), rtol, atol, maxiter, _ptr(self._ws), dev, s))
            return
        if self._spai is not None:
            B.check(B.lib().wlsqm_hip_krylov_spai_start_device(*self._system(transpose), *self._spai_args(transpose), _ptr(b), _ptr(x),
                                                               rtol, atol, maxiter, _ptr(self._ws), dev, s))
            return
        if self._l2:
            B.check(B.lib().wlsqm_hip_krylov_l2_start_device(*self._system(transpose), *self._precond_args(transpose), _ptr(b), _ptr(x),
                                                             rtol, atol, maxiter, _ptr(self._ws), dev, s))
            return
        if self._block is not None:
            B.check(B.lib().wlsqm_hip_krylov_block_start_device(*self._system(transpose), *self._block_args(transpose), _ptr(b), _ptr(x),
                                                                rtol, atol, maxiter, _ptr(self._ws), dev, s))
            return
        B.check(B.lib().wlsqm_hip_krylov_start_device(*self._system(transpose), self._jacobi, _ptr(b), _ptr(x), rtol, atol, maxiter,
                                                      _ptr(self._ws), dev, s))

    def _iterate(self, x, niter, dev, s, transpose=False):
        if self._schwarz is not None:                                    # iterations, or ceil(niter / 2) cycles
            B.check(B.lib().wlsqm_hip_krylov_schwarz_iterate_device(*self._system(transpose), int(self._l2), *self._schwarz_args(transpose),
                                                                    _ptr(x), (niter + 1) // 2 if self._l2 else niter, _ptr(self._ws),
                                                                    dev, s))
            return
        if self._spai is not None:                                       # iterations, or ceil(niter / 2) cycles
            B.check(B.lib().wlsqm_hip_krylov_spai_iterate_device(*self._system(transpose), *self._spai_args(transpose), _ptr(x),
                                                                 (niter + 1) // 2 if self._l2 else niter, _ptr(self._ws), dev, s))
            return
        if self._l2:                                                     # a cycle is two iterations: ceil(niter / 2) cycles
            B.check(B.lib().wlsqm_hip_krylov_l2_device(*self._system(transpose), *self._precond_args(transpose), _ptr(x), (niter + 1) // 2,
                                                       _ptr(self._ws), dev, s))
            return
        if self._block is not None:
            B.check(B.lib().wlsqm_hip_krylov_block_bicgstab_device(*self._system(transpose), *self._block_args(transpose), _ptr(x), niter,
                                                                   _ptr(self._ws), dev, s))
            return
        B.check(B.lib().wlsqm_hip_krylov_bicgstab_device(*self._system(transpose), self._jacobi, _ptr(x), niter, _ptr(self._ws), dev, s))

    def enqueue(self, b, x, iterations, rtol=1e-10, atol=0.0, stream=None, transpose=False):
        """The start of a solve and `iterations` iterations, as kernel launches on `stream` (default: torch's current stream) and nothing
        else: no allocation, no host read, so it can be captured into a graph, also behind op.update(S, check=False).  The solve stops
        by itself, on the device, at ||r|| <= max(rtol ||b||, atol), after `iterations` (status 1) or at a breakdown; what is enqueued
        behind the stop leaves x and the scalars untouched.  x (npoints,) holds the initial guess and receives the solution.
        info() tells later how it went.

        transpose=True solves M^T x = b, M^T = diag(d) + scale * A_o^T, by the same kernels on the operator's transposed matrix (the
        Jacobi diagonal is the same numbers).  That matrix is built at the first transposed use, which allocates and synchronises
        (RuntimeError inside a capture: call op.prepare_transpose() first); op.update keeps it refreshed."""
        self._vectors(b=b, x=x)
        rtol, atol, iterations = self._tolerances(rtol, atol, iterations)
        transpose = self._transposed(transpose, stream)
        s, dev = _stream_and_device(x, stream)
        self._start(b, x, rtol, atol, iterations, dev, s, transpose)
        self._iterate(x, iterations, dev, s, transpose)
        return self

    def _read(self, what, stream):
        """(SolveInfo, done) from the scalars: one read of 128 bytes, which synchronises with the stream."""
        self._live()
        self._no_capture(what, stream)
        with _torch_stream(stream, self._device):
            head = self._ws[:16].cpu().numpy()
        ints = head[8:10].view("int32")
        return SolveInfo(int(ints[1]), int(ints[0]), float(head[4]) ** 0.5), bool(ints[2])

    def info(self, stream=None):
        """SolveInfo of the last solve enqueued on `stream`: one read of 128 bytes, which synchronises with that stream (RuntimeError
        inside a graph capture)."""
        return self._read("info", stream)[0]

    def solve(self, b, x, rtol=1e-10, atol=0.0, maxiter=1000, check_every=8, stream=None, transpose=False):
        """x <- the solution of M x = b from the initial guess in x; returns SolveInfo(status, iterations, residual).  Enqueues
        `check_every` iterations, reads the scalars (one synchronisation) and repeats, up to `maxiter` iterations in all.  The stop is
        taken on the device after every iteration, so `iterations` is exact whatever check_every is; with check_every=1 no launch is
        enqueued behind the stop either.  RuntimeError inside a graph capture.  transpose=True: M^T x = b, as enqueue."""
        self._vectors(b=b, x=x)
        rtol, atol, maxiter = self._tolerances(rtol, atol, maxiter)
        check_every = int(check_every)
        if check_every < 1:
            raise ValueError("check_every must be >= 1; got %d" % check_every)
        self._no_capture("solve", stream)
        transpose = self._transposed(transpose, stream)
        s, dev = _stream_and_device(x, stream)
        self._start(b, x, rtol, atol, maxiter, dev, s, transpose)
        left = maxiter
        while True:
            n = min(check_every, left)
            self._iterate(x, n, dev, s, transpose)
            left -= min(left, n + n % 2) if self._l2 else n
            info, done = self._read("solve", stream)
            if done or left == 0:
                return info

    def product(self, v, w=None, out=None, stream=None, transpose=False):
        """(M v, (M v, w), (M v, M v)): the solve's own fused product and the dot products of its pass (w default v), for checks and
        for residuals.  One host read of the two sums; not between an enqueue and the end of its solve.  transpose=True: M^T v."""
        import torch
        self._live()
        self._no_capture("product", stream)
        w = v if w is None else w
        if out is None:
            with _torch_stream(stream, self._device):
                out = torch.empty((self.npoints,), dtype=torch.float64, device=self._device)
        if w is v:
            self._vectors(v=v, out=out)
        else:
            self._vectors(v=v, w=w, out=out)
        transpose = self._transposed(transpose, stream)
        s, dev = _stream_and_device(v, stream)
        B.check(B.lib().wlsqm_hip_krylov_product_device(*self._system(transpose), _ptr(v), _ptr(w), _ptr(out), _ptr(self._ws), dev, s))
        with _torch_stream(stream, self._device):
            head = self._ws[:16].cpu().numpy()
        return out, float(head[6]), float(head[7])

    # ---- stacked right-hand sides ----

    def _field_tensor(self, t, name, written):
        if not hasattr(t, "dim") or not hasattr(t, "is_cuda"):
            raise ValueError("argument %s must be a device (HIP) tensor" % name)
        _check(t, name, "float64", 2)
        if tuple(t.shape) != (self.nfields, self.npoints):
            raise ValueError("%s must be a float64 device tensor of shape (%d, %d), one row per field of the solver (nfields = %d); got "
                             "shape %s" % (name, self.nfields, self.npoints, self.nfields, tuple(t.shape)))
        if t.device != self._device:
            raise ValueError("all tensors must be on the same device")
        sf, sp = (abs(st) for st in t.stride())
        if written and not ((self.nfields == 1 or sf >= self.npoints * sp) and (self.npoints == 1 or sp > 0)
                            or (self.npoints == 1 or sp >= self.nfields * sf) and (self.nfields == 1 or sf > 0)):
            raise ValueError("the elements of %s must be distinct in memory; got strides %s" % (name, tuple(t.stride())))

    def _fields(self, written=(), **named):
        """The checks of the stacked arrays of a call: each one (nfields, npoints) float64 on the operator's device, with any strides
        (those named in `written`: no two elements in one place), none overlapping another, the diag tensor or the workspace."""
        self._live()
        for name, t in named.items():
            self._field_tensor(t, name, name in written)
        self._disjoint(named)

    @staticmethod
    def _strided(t):
        return _ptr(t), t.stride(0), t.stride(1)

    def _precond_args(self, transpose=False):
        if self._block is not None:
            return self._block_args(transpose)
        return self._jacobi, None

    def _start_many(self, b, x, rtol, atol, maxiter, dev, s, transpose=False):
        if self._block is not None:
            self._factor(dev, s, transpose)
        B.check(B.lib().wlsqm_hip_krylov_many_start_device(*self._system(transpose), self.nfields, *self._strided(b), *self._strided(x),
                                                           *self._precond_args(transpose), rtol, atol, maxiter, _ptr(self._ws), dev, s))

    def _iterate_many(self, x, niter, dev, s, transpose=False):
        B.check(B.lib().wlsqm_hip_krylov_many_bicgstab_device(*self._system(transpose), self.nfields, *self._strided(x),
                                                              *self._precond_args(transpose), niter, _ptr(self._ws), dev, s))

    def enqueue_many(self, b, x, iterations, rtol=1e-10, atol=0.0, stream=None, transpose=False):
        """enqueue for nfields right-hand sides at once: b and x (nfields, npoints) float64 with any strides, row f of x the initial
        guess and the solution of M x_f = b_f.  The fields are independent solves — field f's x, iteration count, status and residual
        are, bit for bit, those of enqueue on b[f], x[f] alone — that share the launches and every pass over the matrix; each stops
        by its own threshold max(rtol ||b_f||, atol) or breakdown and is left untouched from then on while the others go on.
        Launches only, as enqueue: capturable, also behind op.update(S, check=False).  info_many() tells later how it went."""
        self._fields(written=("x",), b=b, x=x)
        rtol, atol, iterations = self._tolerances(rtol, atol, iterations)
        if self.nfields == 1:
            return self.enqueue(b[0], x[0], iterations, rtol=rtol, atol=atol, stream=stream, transpose=transpose)
        transpose = self._transposed(transpose, stream)
        s, dev = _stream_and_device(x, stream)
        self._start_many(b, x, rtol, atol, iterations, dev, s, transpose)
        self._iterate_many(x, iterations, dev, s, transpose)
        return self

    def _read_many(self, what, stream):
        """([SolveInfo per field], all done) from the heads: one read of 8 x 128 + 8 bytes, which synchronises with the stream."""
        self._live()
        if self.nfields == 1:
            info, done = self._read(what, stream)
            return [info], done
        self._no_capture(what, stream)
        with _torch_stream(stream, self._device):
            head = self._ws[:129].cpu().numpy()
        infos = []
        for f in range(self.nfields):
            h = head[16 * f:16 * f + 16]
            ints = h[8:10].view("int32")
            infos.append(SolveInfo(int(ints[1]), int(ints[0]), float(h[4]) ** 0.5))
        return infos, bool(head[128:129].view("int32")[0])

    def info_many(self, stream=None):
        """The SolveInfo of every field of the last solve_many / enqueue_many on `stream`, as a list: one read, which synchronises with
        that stream (RuntimeError inside a graph capture)."""
        return self._read_many("info_many", stream)[0]

    def solve_many(self, b, x, rtol=1e-10, atol=0.0, maxiter=1000, check_every=8, stream=None, transpose=False):
        """solve for nfields right-hand sides at once (enqueue_many says what that means): returns the list of SolveInfo, one per field.
        Enqueues `check_every` iterations, reads the heads (one synchronisation) and repeats until every field has stopped, up to
        `maxiter` iterations.  RuntimeError inside a graph capture."""
        self._fields(written=("x",), b=b, x=x)
        rtol, atol, maxiter = self._tolerances(rtol, atol, maxiter)
        check_every = int(check_every)
        if check_every < 1:
            raise ValueError("check_every must be >= 1; got %d" % check_every)
        self._no_capture("solve_many", stream)
        if self.nfields == 1:
            return [self.solve(b[0], x[0], rtol=rtol, atol=atol, maxiter=maxiter, check_every=check_every, stream=stream, transpose=transpose)]
        transpose = self._transposed(transpose, stream)
        s, dev = _stream_and_device(x, stream)
        self._start_many(b, x, rtol, atol, maxiter, dev, s, transpose)
        left = maxiter
        while True:
            n = min(check_every, left)
            self._iterate_many(x, n, dev, s, transpose)
            left -= n
            infos, done = self._read_many("solve_many", stream)
            if done or left == 0:
                return infos

    def product_many(self, v, w=None, out=None, stream=None, transpose=False):
        """product for nfields vectors at once: (out, [(M v_f, w_f)], [(M v_f, M v_f)]), out (nfields, npoints) = M v per field, each
        field's numbers bit for bit those of product on v[f], w[f] alone (w default v).  v, w and out take any strides.  One host read;
        not between an enqueue_many and the end of its solve."""
        import torch
        self._live()
        self._no_capture("product_many", stream)
        w = v if w is None else w
        if out is None:
            with _torch_stream(stream, self._device):
                out = torch.empty((self.nfields, self.npoints), dtype=torch.float64, device=self._device)
        if w is v:
            self._fields(written=("out",), v=v, out=out)
        else:
            self._fields(written=("out",), v=v, w=w, out=out)
        if self.nfields == 1:
            _, dot_w, dot_v = self.product(v[0], None if w is v else w[0], out=out[0], stream=stream, transpose=transpose)
            return out, [dot_w], [dot_v]
        transpose = self._transposed(transpose, stream)
        s, dev = _stream_and_device(v, stream)
        B.check(B.lib().wlsqm_hip_krylov_many_product_device(*self._system(transpose), self.nfields, *self._strided(v), *self._strided(w),
                                                             *self._strided(out), _ptr(self._ws), dev, s))
        with _torch_stream(stream, self._device):
            head = self._ws[:128].cpu().numpy()
        return out, [float(head[16 * f + 6]) for f in range(self.nfields)], [float(head[16 * f + 7]) for f in range(self.nfields)]

    def gradients(self, lam, x, values=False, diag=False, scale=False, stream=None):
        """The gradients of a loss L through the solve M x = b, from x and lam, the solution of M^T lam = dL/dx (solve(transpose=True)):
        SolveGradients(values, diag, scale), each None unless asked for with True or with a tensor to write into.
          values: (total,) in the operator's layout, -((scale * lam_j) * x_col) at every live entry of row j, +0.0 in the padding:
                  dL/d(the entries of value plane o); op.unpack(values) gives it per slot.
          diag:   (npoints,), -(lam_i * x_i): dL/d(diag).
          scale:  a 0-d device tensor, -(lam, A_o x): dL/d(scale), copied from the workspace on the stream (no host read).
        One kernel launch on `stream` ("krylov-grads": one pass over the forward matrix), and the one-workgroup reduce for `scale`;
        no synchronisation, no allocation when the outputs are given.  lam, x and the outputs are contiguous float64 tensors on the
        operator's device that overlap neither each other nor the diag tensor, the operator's values or the workspace.  Like product,
        not between an enqueue and the end of its solve."""
        import torch
        m = self._live()
        total = int(m["total"])
        asked = lambda flag: flag is not None and flag is not False
        if not (asked(values) or asked(diag) or asked(scale)):
            raise ValueError("gradients: none of values, diag and scale is asked for")
        f64 = dict(dtype=torch.float64, device=self._device)
        with _torch_stream(stream, self._device):
            gval = torch.empty((total,), **f64) if values is True else (values if asked(values) else None)
            gdiag = torch.empty((self.npoints,), **f64) if diag is True else (diag if asked(diag) else None)
            gscale = torch.empty((), **f64) if scale is True else (scale if asked(scale) else None)
        named = dict(lam=lam, x=x)
        if gdiag is not None:
            named["grad_diag"] = gdiag
        self._vectors(**named)
        others = dict(named, workspace=self._ws, **{"the operator's values": self._op._val})
        if hasattr(self.diag, "dim"):
            others["diag"] = self.diag
        for t, name, shape in ((gval, "values", (total,)), (gscale, "scale", None)):
            if t is None:
                continue
            if not hasattr(t, "dim") or not hasattr(t, "is_cuda"):
                raise ValueError("argument %s must be True, False or a device (HIP) tensor" % name)
            if shape is None:
                if str(t.dtype) != "torch.float64" or not t.is_cuda or t.numel() != 1:
                    raise ValueError("scale must be a float64 device tensor of one element; got %s of shape %s" % (t.dtype, tuple(t.shape)))
            else:
                _check(t, name, "float64", 1)
                if tuple(t.shape) != shape or (total > 1 and t.stride(0) != 1):
                    raise ValueError("%s must be a contiguous float64 device tensor of shape %s, the operator's layout; got shape %s with "
                                     "strides %s" % (name, shape, tuple(t.shape), tuple(t.stride())))
            if t.device != self._device:
                raise ValueError("all tensors must be on the same device")
            for other, held in others.items():
                if _overlap(t, held):
                    raise ValueError("%s overlaps %s in memory" % (name, other))
            others[name] = t
        s, dev = _stream_and_device(x, stream)
        B.check(B.lib().wlsqm_hip_krylov_grads_device(*self._system(), _ptr(lam), _ptr(x), _ptr(gval) if total else None, _ptr(gdiag),
                                                      1 if gscale is not None else 0, _ptr(self._ws), dev, s))
        if gscale is not None:
            with _torch_stream(stream, self._device):
                gscale.view(-1).copy_(self._ws[6:7])
        return SolveGradients(gval, gdiag, gscale)


class StencilSystemSolver:
    """Solves M x = b for m coupled fields on one cloud (1 <= m <= 4): block (a, b) of M is
    D_ab + sum_o coupling[a, b, o] A_o, A_o the value planes of a square StencilOperator, by the device-resident BiCGSTAB of
    StencilSolver: eight launches per iteration, the product one pass over the operator's own planes (4 + 8 nop bytes per neighbour,
    whatever m is) that gathers a neighbour's m unknowns as one contiguous load.  No atomics: the bits of x and of the iteration count
    are a function of the inputs, and eager and captured runs agree.

    op: as StencilSolver takes it — square, row j the equation of point j, not closed, without known derivatives — with at most 8 planes.
    coupling: host array-like of float64 (m, m, nop), every entry finite; read here, once (set_coupling replaces the table).  Or a
    contiguous float64 device tensor (m, m, nop, npoints), plane-major like the diag tensor: the equation of point i
    carries its own coefficients, M[(i, a), (j, b)] = D_ab,i delta_ij + sum_o coupling[a, b, o, i] A_o[i, j].  The tensor is read on the
    stream by every start, product and gradient; the caller may change it in place, and a captured graph sees the change.  Its kernels
    sum in another order than the constant table's (same bounds, other bits); M^T mixes lam with the coefficients at their own point
    into a plane of m nop npoints doubles first (prepare_transpose), 10 launches per iteration.
    diag: a float d (D = d I_m), a host (m, m) array-like of constants, or a contiguous float64 device tensor (m, m, npoints), each
    D_ab a diagonal matrix; a tensor is read at every solve (the caller may change it in place).
    preconditioner: "jacobi", the inverse of the scalar diagonal of M — for unknown (i, a): D_aa,i + sum_o coupling[a, a, o] (the sum of
    row i's own entries in plane o) — None, or a PointBlockJacobi: the exact inverses of the diagonal blocks of
    `points` consecutive points with all m unknowns of each, for a cloud in Morton order; block_points and block_rows say what it
    took.  It brings what a BlockJacobi brings to a StencilSolver, under the same conventions: refresh(), precondition(v),
    preconditioner_blocks(), the transposed plane from prepare_transpose(), status 4 for a block that cannot be inverted.  Its planes
    are wlsqm_hip_krylov_system_block_bytes(npoints, m, points) bytes each.

    Unknowns and right-hand sides are contiguous float64 device tensors (npoints, m): x[i, a] is component a at point i.  For m = 2 and 4
    they are moved by 16-byte loads and must be 16-byte aligned, as every tensor that torch allocates is.
    The workspace is StencilSolver's at m npoints rows, 9 m npoints + 2 ceil(m npoints / 256) + 16 doubles, allocated here.
    solve, enqueue and product take transpose=True for M^T, whose block (a, b) is D_ba + sum_o coupling[b, a, o] A_o^T: the same kernels
    on the operator's transposed arrays (prepare_transpose), a diag tensor read in place.  gradients(), coupling_gradient() and
    differentiable_stencil_system_solve carry a loss through the solve.
    Out of scope (sections 24 to 27): method="bicgstab2", BlockJacobi (its block counts rows) and ApproximateInverse, blocks of more
    than 32 rows, nfields, a coupling that scales columns, m > 4, a capturable backward pass, second derivatives, wlsqm.sharded."""

    def __init__(self, op, coupling, diag=0.0, preconditioner="jacobi"):
        import numpy as np
        import torch
        self._ws = None
        if not isinstance(op, StencilOperator):
            raise ValueError("op must be a StencilOperator")
        op._live()
        if op.ncases != op.npoints:
            raise ValueError("the operator must be square: it has %d rows (cases) for %d points" % (op.ncases, op.npoints))
        if op.has_known_derivatives:
            raise ValueError("the operator depends on known DOFs other than F: their affine term belongs in b, build the operator without them")
        self._block = preconditioner if isinstance(preconditioner, PointBlockJacobi) else None
        if self._block is None and preconditioner is not None and not (isinstance(preconditioner, str) and preconditioner == "jacobi"):
            raise ValueError("preconditioner must be 'jacobi' or None, or a PointBlockJacobi, for coupled fields (its blocks count points; "
                             "a BlockJacobi's count rows); got %r" % (preconditioner,))
        self._jacobi = 1 if self._block is None and preconditioner == "jacobi" else 0
        self._planes = self._planes_t = None
        self._factored = self._factored_t = False
        self.block_points = self.block_rows = None
        self.per_point = self._is_point_table(coupling)
        self._mixed = None
        if self.per_point:
            cp = self._coupling_tensor(coupling, op.nop, op.npoints, op._m["col"])
        else:
            cp = self._coupling_table(coupling, op.nop)
        m = int(cp.shape[0])
        self.m, self.nop, self.npoints, self._device = m, op.nop, op.npoints, op._device
        self.coupling = cp
        if self._block is not None:
            points = 16 // m if self._block.points is None else self._block.points
            if m * points > 32:
                raise ValueError("points must be 1 .. %d for m = %d: a block holds m points <= 32 rows; got %d" % (32 // m, m, points))
            self.block_points, self.block_rows = points, m * points
        if hasattr(diag, "dim"):
            if not hasattr(diag, "is_cuda"):
                raise ValueError("argument diag must be a device (HIP) tensor")
            _check(diag, "diag", "float64", 3)
            if tuple(diag.shape) != (m, m, self.npoints) or not diag.is_contiguous():
                raise ValueError("diag must be a contiguous float64 device tensor of shape (%d, %d, %d); got shape %s with strides %s"
                                 % (m, m, self.npoints, tuple(diag.shape), tuple(diag.stride())))
            _same_device(op._m["col"], diag)
            self.diag, dc = diag, np.zeros((m, m))
        else:
            dc = np.asarray(diag, dtype=np.float64)
            if dc.ndim == 0:
                dc = float(dc) * np.eye(m)
            if dc.shape != (m, m):
                raise ValueError("diag must be a float, a host array (%d, %d) or a device tensor (%d, %d, %d); got shape %s"
                                 % (m, m, m, m, self.npoints, tuple(dc.shape)))
            if not np.isfinite(dc).all():
                raise ValueError("every entry of diag must be finite")
            self.diag = dc = np.ascontiguousarray(dc)
        self._cp = None if self.per_point else (C.c_double * cp.size)(*cp.ravel().tolist())
        self._dc = (C.c_double * (m * m))(*dc.ravel().tolist())
        pi = getattr(op, "_point_index", None)
        if pi is not None and not bool((pi[:op.ncases].long() == torch.arange(op.ncases, device=pi.device)).all()):
            raise ValueError("row j of the operator must be the equation of point j: point_index must be None or the identity")
        self._op = op
        self.x = None
        nbytes = int(B.lib().wlsqm_hip_krylov_system_workspace_bytes(self.npoints, m))
        self._ws = torch.zeros((nbytes // 8,), dtype=torch.float64, device=self._device)
        if self._block is not None:
            self._planes = self._new_planes()

    def _new_planes(self):
        import torch
        nbytes = int(B.lib().wlsqm_hip_krylov_system_block_bytes(self.npoints, self.m, self.block_points))
        return torch.zeros((nbytes // 8,), dtype=torch.float64, device=self._device)

    @staticmethod
    def _coupling_table(coupling, nop, m=None):
        """The constructor's checks of `coupling`: a contiguous float64 host array (m, m, nop), every entry finite (m given: that m)."""
        import numpy as np
        if hasattr(coupling, "is_cuda") and coupling.is_cuda:
            raise ValueError("coupling must be a host array (m, m, nop); got a device tensor")
        cp = np.ascontiguousarray(np.array(coupling, dtype=np.float64))    # a copy: the caller's array may change afterwards
        if cp.ndim != 3 or cp.shape[0] != cp.shape[1] or not 1 <= cp.shape[0] <= 4 or cp.shape[2] != nop:
            raise ValueError("coupling must have shape (m, m, nop) with 1 <= m <= 4 and nop = %d, the operator's value planes; got shape %s"
                             % (nop, tuple(cp.shape)))
        if nop > 8:
            raise ValueError("coupled fields take an operator of at most 8 value planes; it has %d" % nop)
        if m is not None and cp.shape[0] != m:
            raise ValueError("the new coupling must keep the solver's shape (%d, %d, %d); got shape %s" % (m, m, nop, tuple(cp.shape)))
        if not np.isfinite(cp).all():
            raise ValueError("every entry of coupling must be finite")
        return cp

    @staticmethod
    def _is_point_table(coupling):
        """True for what is taken as a per-point table: a device tensor of four dimensions.  A device tensor of any other rank is left
        to _coupling_table, which refuses it."""
        return bool(hasattr(coupling, "is_cuda") and coupling.is_cuda and hasattr(coupling, "dim") and coupling.dim() == 4)

    @staticmethod
    def _coupling_tensor(coupling, nop, npoints, like, m=None):
        """The constructor's checks of a per-point `coupling`: a contiguous float64 device tensor (m, m, nop, npoints) on the operator's
        device (m given: that m).  Its entries are not read here: a NaN or Inf among them ends a solve with status 3 or 4."""
        _check(coupling, "coupling", "float64", 4)
        sh = tuple(coupling.shape)
        if sh[0] != sh[1] or not 1 <= sh[0] <= 4 or sh[2] != nop or sh[3] != npoints or not coupling.is_contiguous():
            raise ValueError("a per-point coupling must be a contiguous float64 device tensor of shape (m, m, nop, npoints) with 1 <= m <= 4, "
                             "nop = %d, the operator's value planes, and npoints = %d; got shape %s with strides %s"
                             % (nop, npoints, sh, tuple(coupling.stride())))
        if nop > 8:
            raise ValueError("coupled fields take an operator of at most 8 value planes; it has %d" % nop)
        if m is not None and sh[0] != m:
            raise ValueError("the new coupling must keep the solver's shape (%d, %d, %d, %d); got shape %s" % (m, m, nop, npoints, sh))
        _same_device(like, coupling)
        return coupling

    def set_coupling(self, coupling):
        """Replace the coupling table by a new one of the same kind and shape, under the constructor's checks (ValueError).
        A host table (m, m, nop) is host memory that travels with every launch: nothing is enqueued, and the next solve, product or
        gradient reads the new one (a captured graph keeps the table it was captured with) — parameter sweeps on one workspace, and
        what autograd writes `coupling` with.  A per-point solver takes a new device tensor (m, m, nop, npoints) on the same device,
        which the next call reads on its stream; a captured graph keeps reading the tensor it was captured with, whose contents the
        caller may change in place.  Changing a solver from one kind of table to the other is a ValueError."""
        self._live()
        if self._is_point_table(coupling) != self.per_point:
            raise ValueError("set_coupling cannot change the kind of table: the solver was made with %s"
                             % ("a per-point device tensor (m, m, nop, npoints)" if self.per_point else "a host table (m, m, nop)"))
        if self.per_point:
            self.coupling = self._coupling_tensor(coupling, self.nop, self.npoints, self._ws, self.m)
            return self
        cp = self._coupling_table(coupling, self.nop, self.m)
        self.coupling = cp
        self._cp = (C.c_double * cp.size)(*cp.ravel().tolist())
        return self

    def _live(self):
        if getattr(self, "_ws", None) is None:
            raise RuntimeError("the stencil system solver has been closed")
        return self._op._live()

    def close(self):
        """Release the workspace now; harmless when called again.  The operator and a diag tensor stay the caller's."""
        self._ws = self._op = self.x = self._mixed = self._planes = self._planes_t = None
        if hasattr(self.__dict__.get("diag"), "dim"):
            self.diag = None
        if self.__dict__.get("per_point"):
            self.coupling = None

    def memory_used(self):
        """Bytes of device memory the solver holds: the workspace and, for a per-point coupling once a transposed use has allocated
        it, the mixed plane of m nop npoints doubles, and the planes of a PointBlockJacobi (wlsqm_hip_krylov_system_block_bytes each; the
        transposed one from the first transposed use on).  The coupling tensor is the caller's."""
        self._live()
        return sum(t.numel() * t.element_size() for t in (self._ws, self._mixed, self._planes, self._planes_t) if t is not None)

    def refresh(self, stream=None):
        """The Jacobi diagonal is recomputed from the operator's arrays and the diag tensor as they are on the stream by the start of
        every solve and enqueue, a captured one included: after op.update or an in-place change of diag there is nothing left to call.
        refresh() says so in code that is written for a preconditioner which needs it; it checks that the solver is live.
        With a PointBlockJacobi: its blocks are recomputed now from the operator's arrays, coupling and diag as they are on `stream` —
        what refresh=False leaves to the caller.  One kernel launch ("krylov-system-blocks"), no allocation, no host read: capturable."""
        self._live()
        if self._block is not None:
            s, dev = _stream_and_device(self._planes, stream)
            self._factor(dev, s, force=True)
        return self

    def _factor(self, dev, s, transpose=False, force=False):
        """"krylov-system-blocks" when P is due, by StencilSolver._factor's rules: at every start with refresh=True, else at the first one,
        when the transposed plane is new, and from refresh().  One launch on the forward arrays, the forward coupling and diag, which
        fills the transposed plane too when this start needs it or, with refresh=False, whenever it exists."""
        bj = self._block
        if not (force or bj.refresh or not self._factored or (transpose and not self._factored_t)):
            return
        both = self._planes_t is not None and (transpose or not bj.refresh or force)
        B.check(B.lib().wlsqm_hip_krylov_system_block_factor_device(*self._system(False)[:13], 1 if self.per_point else 0, self.block_points,
                                                                    _ptr(self._planes), _ptr(self._planes_t) if both else None, dev, s))
        self._factored = True
        if both:
            self._factored_t = True
        elif bj.refresh:
            self._factored_t = False

    def _block_args(self, transpose=False):
        return self.block_points, _ptr(self._planes_t if transpose else self._planes)

    def precondition(self, v, out=None, stream=None, transpose=False):
        """z = P v (P^T v with transpose=True) on (npoints, m) tensors, P the PointBlockJacobi's block inverses as the next solve would
        use them: factored first when due (refresh=True: always).  One launch ("krylov-system-precondition") behind the factor's; v and
        out must not overlap.  ValueError on a solver without blocks."""
        import torch
        self._live()
        if self._block is None:
            raise ValueError("precondition() belongs to a PointBlockJacobi preconditioner")
        if out is None:
            with _torch_stream(stream, self._device):
                out = torch.empty((self.npoints, self.m), dtype=torch.float64, device=self._device)
        self._vectors(v=v, out=out)
        transpose = self._transposed(transpose, stream)
        s, dev = _stream_and_device(v, stream)
        self._factor(dev, s, transpose)
        B.check(B.lib().wlsqm_hip_krylov_system_block_precondition_device(self.npoints, self.m, *self._block_args(transpose), _ptr(v),
                                                                          _ptr(out), dev, s))
        return out

    def _blocks_of(self, plane):
        """(nblocks, R, R) out of a plane in the layout of section 27, as a new tensor."""
        rows = self.block_rows
        nb = 8 if rows <= 8 else 16 if rows <= 16 else 32
        nblocks = (self.npoints + self.block_points - 1) // self.block_points
        nwaves = (nblocks * nb + 63) // 64
        W = plane[:nwaves * nb * 64].view(nwaves, nb, 64 // nb, nb)                      # [wave, j, g, l]
        return W.permute(0, 2, 3, 1).reshape(-1, nb, nb)[:nblocks, :rows, :rows].clone()

    def _matrix_blocks(self, stream=None):
        """Internal check hook (the tests hold the gather to its bound through it; not part of the supported surface): the
        diagonal blocks of M themselves, (nblocks, R, R), as the factor gathers them from the operator's arrays, coupling and
        diag before it inverts them ("krylov-system-blocks" without the elimination, into a plane of its own): for checks.  It
        allocates, so it is not for a graph capture."""
        self._live()
        if self._block is None:
            raise ValueError("_matrix_blocks() belongs to a PointBlockJacobi preconditioner")
        s, dev = _stream_and_device(self._planes, stream)
        with _torch_stream(stream, self._device):
            plane = self._new_planes()
            B.check(B.lib().wlsqm_hip_krylov_system_block_gather_device(*self._system(False)[:13], 1 if self.per_point else 0,
                                                                        self.block_points, _ptr(plane), dev, s))
            return self._blocks_of(plane)

    def preconditioner_blocks(self, transpose=False, stream=None):
        """The inverse blocks (of M^T with transpose=True) as a new tensor (nblocks, R, R), nblocks = ceil(npoints / block_points) and
        R = block_rows, factored first when due; what the cut last block leaves over is the identity.  It allocates the result, so
        it is not for a graph capture."""
        self._live()
        if self._block is None:
            raise ValueError("preconditioner_blocks() belongs to a PointBlockJacobi preconditioner")
        transpose = self._transposed(transpose, stream)
        s, dev = _stream_and_device(self._planes, stream)
        self._factor(dev, s, transpose)
        with _torch_stream(stream, self._device):
            return self._blocks_of(self._planes_t if transpose else self._planes)

    def _vector(self, t, name):
        if not hasattr(t, "dim") or not hasattr(t, "is_cuda"):
            raise ValueError("argument %s must be a device (HIP) tensor" % name)
        _check(t, name, "float64", 2)
        if tuple(t.shape) != (self.npoints, self.m) or not t.is_contiguous():
            raise ValueError("%s must be a contiguous float64 device tensor of shape (%d, %d), the m unknowns of a point side by side; got "
                             "shape %s with strides %s" % (name, self.npoints, self.m, tuple(t.shape), tuple(t.stride())))
        _same_device(self._ws, t)
        if self.m % 2 == 0 and t.data_ptr() % 16:
            raise ValueError("%s must be 16-byte aligned for m = %d" % (name, self.m))

    def _vectors(self, **named):
        self._live()
        for name, t in named.items():
            self._vector(t, name)
        held = dict(named, workspace=self._ws)
        if hasattr(self.diag, "dim"):
            held["diag"] = self.diag
        if self.per_point:
            held["coupling"] = self.coupling
            if self._mixed is not None:
                held["the mixed plane"] = self._mixed
        for name, t in (("the preconditioner's blocks", self._planes), ("the preconditioner's transposed blocks", self._planes_t)):
            if t is not None:
                held[name] = t
        names = list(held)
        for i, a in enumerate(names):
            for b in names[i + 1:]:
                if a in named and _overlap(held[a], held[b]):
                    raise ValueError("%s overlaps %s in memory" % (a, b))

    def _system(self, transpose=False):
        """The system's arguments of the C entry points; transpose: the operator's transposed arrays for the *_transposed_device calls,
        which exchange (a, b) in coupling and diag themselves.  A per-point solver: the coupling tensor's pointer in the table's place,
        then `transposed` and the mixed plane, the leading arguments of the *_point_* calls."""
        m, val = (self._op._t, self._op._tval) if transpose else (self._op._m, self._op._val)
        d = self.diag
        head = (m["nrows"], int(m["width"].shape[0]), _ptr(m["len"]), _ptr(m["width"]), _ptr(m["soff"]), _ptr(m["col"]), _ptr(val),
                m["total"], self.nop, self.m)
        tail = (_ptr(d) if hasattr(d, "dim") else None, C.cast(self._dc, C.c_void_p))
        if self.per_point:
            return head + (_ptr(self.coupling),) + tail + (1 if transpose else 0, _ptr(self._mixed) if transpose else None)
        return head + (C.cast(self._cp, C.c_void_p),) + tail

    def _call(self, what, transpose, block=False):
        """The C entry point of `what` (start, bicgstab, product) for this solver's kind of table; block: the form that takes the
        blocks of a PointBlockJacobi (start, bicgstab)."""
        what = "block_" + what if block else what
        if self.per_point:
            return getattr(B.lib(), "wlsqm_hip_krylov_system_point_%s_device" % what)
        return getattr(B.lib(), "wlsqm_hip_krylov_system_%s%s_device" % (what, "_transposed" if transpose else ""))

    _no_capture = StencilSolver._no_capture
    _tolerances = staticmethod(StencilSolver._tolerances)

    def _transposed(self, transpose, stream):
        """The operator's transposed matrix and a per-point solver's mixed plane, built at the first transposed use (prepare_transpose:
        RuntimeError inside a capture)."""
        if transpose and (self._op._t is None or (self.per_point and self._mixed is None)
                          or (self._block is not None and self._planes_t is None)):
            self.prepare_transpose(stream)
        return bool(transpose)

    def prepare_transpose(self, stream=None):
        """Build now what a transposed solve needs: the operator's transposed matrix with all its planes (op.prepare_transpose).  Without
        this call the first transposed use builds it, which allocates and synchronises — RuntimeError when that would happen inside a
        graph capture.  op.update and set_coefficients keep it refreshed, or drop it where the operator does (new hoods; too large for
        its index pairs), and the next transposed use rebuilds it.  Returns True when this call built something."""
        self._live()
        built = self._op.prepare_transpose(stream) if self._op._t is None else False
        if self.per_point and self._mixed is None:
            import torch
            with _torch_stream(stream, self._device):
                if self._device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("the solver has no mixed plane for its per-point coupling yet and the stream is capturing: call "
                                       "prepare_transpose before the capture")
                self._mixed = torch.zeros((self.npoints, self.nop, self.m), dtype=torch.float64, device=self._device)
            built = True
        if self._block is not None and self._planes_t is None:
            import torch
            with _torch_stream(stream, self._device):
                if self._device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("the solver has no transposed preconditioner blocks yet and the stream is capturing: call "
                                       "prepare_transpose before the capture")
                self._planes_t = self._new_planes()
            self._factored_t = False
            built = True
        return built

    def _start(self, b, x, rtol, atol, maxiter, dev, s, transpose=False):
        if self._block is not None:
            self._factor(dev, s, transpose)
            B.check(self._call("start", transpose, True)(*self._system(transpose), *self._block_args(transpose), _ptr(b), _ptr(x), rtol,
                                                         atol, maxiter, _ptr(self._ws), dev, s))
            return
        B.check(self._call("start", transpose)(*self._system(transpose), self._jacobi, _ptr(b), _ptr(x), rtol, atol, maxiter,
                                               _ptr(self._ws), dev, s))

    def _iterate(self, x, niter, dev, s, transpose=False):
        if self._block is not None:
            B.check(self._call("bicgstab", transpose, True)(*self._system(transpose), *self._block_args(transpose), _ptr(x), niter,
                                                            _ptr(self._ws), dev, s))
            return
        B.check(self._call("bicgstab", transpose)(*self._system(transpose), self._jacobi, _ptr(x), niter, _ptr(self._ws), dev, s))

    def enqueue(self, b, x, iterations, rtol=1e-10, atol=0.0, stream=None, transpose=False):
        """The start of a solve and `iterations` iterations as kernel launches on `stream` and nothing else, as StencilSolver.enqueue:
        no allocation, no host read, capturable behind op.update(S, check=False).  x (npoints, m) holds the initial guess and receives
        the solution; info() tells later how it went.  transpose=True solves M^T x = b by the same kernels on the operator's transposed
        matrix, which is built at the first transposed use (RuntimeError inside a capture: call prepare_transpose first)."""
        self._vectors(b=b, x=x)
        rtol, atol, iterations = self._tolerances(rtol, atol, iterations)
        transpose = self._transposed(transpose, stream)
        s, dev = _stream_and_device(x, stream)
        self._start(b, x, rtol, atol, iterations, dev, s, transpose)
        self._iterate(x, iterations, dev, s, transpose)
        self.x = x
        return self

    def _read(self, what, stream):
        self._live()
        self._no_capture(what, stream)
        with _torch_stream(stream, self._device):
            head = self._ws[:16].cpu().numpy()
        ints = head[8:10].view("int32")
        return SolveInfo(int(ints[1]), int(ints[0]), float(head[4]) ** 0.5), bool(ints[2])

    def info(self, stream=None):
        """SolveInfo of the last solve enqueued on `stream`: one read of 128 bytes, which synchronises with that stream."""
        return self._read("info", stream)[0]

    def solve(self, b, x0=None, rtol=1e-10, atol=0.0, maxiter=1000, check_every=8, stream=None, transpose=False):
        """The solution of M x = b; returns SolveInfo(status, iterations, residual).  x0 (npoints, m) is what StencilSolver.solve calls
        x: it holds the initial guess and receives the solution in place.  x0=None starts from zero in a new tensor.  Either way
        `solver.x` names the tensor that holds the solution afterwards.  The outcome is read every `check_every` iterations; the stop
        is taken on the device after every iteration.  RuntimeError inside a graph capture.  transpose=True: M^T x = b, as enqueue."""
        import torch
        self._live()
        self._no_capture("solve", stream)
        if x0 is None:
            with _torch_stream(stream, self._device):
                x0 = torch.zeros((self.npoints, self.m), dtype=torch.float64, device=self._device)
        x = x0
        self._vectors(b=b, x=x)
        rtol, atol, maxiter = self._tolerances(rtol, atol, maxiter)
        check_every = int(check_every)
        if check_every < 1:
            raise ValueError("check_every must be >= 1; got %d" % check_every)
        transpose = self._transposed(transpose, stream)
        s, dev = _stream_and_device(x, stream)
        self._start(b, x, rtol, atol, maxiter, dev, s, transpose)
        self.x = x
        left = maxiter
        while True:
            n = min(check_every, left)
            self._iterate(x, n, dev, s, transpose)
            left -= n
            info, done = self._read("solve", stream)
            if done or left == 0:
                return info

    def product(self, v, w=None, out=None, stream=None, transpose=False):
        """(M v, (M v, w), (M v, M v)): the solve's own fused product and the dot products of its pass (w default v), all (npoints, m).
        One host read of the two sums; not between an enqueue and the end of its solve.  transpose=True: M^T v."""
        import torch
        self._live()
        self._no_capture("product", stream)
        w = v if w is None else w
        if out is None:
            with _torch_stream(stream, self._device):
                out = torch.empty((self.npoints, self.m), dtype=torch.float64, device=self._device)
        if w is v:
            self._vectors(v=v, out=out)
        else:
            self._vectors(v=v, w=w, out=out)
        transpose = self._transposed(transpose, stream)
        s, dev = _stream_and_device(v, stream)
        B.check(self._call("product", transpose)(*self._system(transpose), _ptr(v), _ptr(w), _ptr(out), _ptr(self._ws), dev, s))
        with _torch_stream(stream, self._device):
            head = self._ws[:16].cpu().numpy()
        return out, float(head[6]), float(head[7])

    def matrix(self):
        """M as a new torch.sparse_csr_tensor of m npoints rows in the interleaved numbering (row i m + a: component a at point i), built
        with torch operations from the operator's planes, coupling and diag as they are now: columns sorted, duplicates summed, the
        blocks whose coupling is all zeros left out.  A per-point coupling scales the entries of row i by coupling[a, b, :, i] (one host
        read per block to see whether it is all zeros).  For checks and as the baseline of a flattened solve; not for a graph capture."""
        import torch
        self._live()
        op, m, n = self._op, self.m, self.npoints
        src, row = op._entries()
        col = op._m["col"][src].long()
        rows, cols, vals = [], [], []
        cp = self.coupling if self.per_point else torch.from_numpy(self.coupling).to(self._device)
        for a in range(m):
            for b in range(m):
                if bool((cp if self.per_point else self.coupling)[a, b].any()):
                    rows.append(row * m + a)
                    cols.append(col * m + b)
                    vals.append(((cp[a, b][:, row] if self.per_point else cp[a, b][:, None]) * op._val[:, src]).sum(dim=0))
                tensor = hasattr(self.diag, "dim")
                if tensor or self.diag[a, b] != 0.0:
                    i = torch.arange(n, device=self._device)
                    rows.append(i * m + a)
                    cols.append(i * m + b)
                    vals.append(self.diag[a, b] if tensor else torch.full((n,), float(self.diag[a, b]), dtype=torch.float64, device=self._device))
        if not rows:
            rows = cols = [torch.zeros((0,), dtype=torch.int64, device=self._device)]
            vals = [torch.zeros((0,), dtype=torch.float64, device=self._device)]
        coo = torch.sparse_coo_tensor(torch.stack([torch.cat(rows), torch.cat(cols)]), torch.cat(vals), (m * n, m * n))
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            return coo.coalesce().to_sparse_csr()

    def gradients(self, lam, x, values=False, diag=False, stream=None):
        """The gradients of a loss L through the solve M x = b, from x and lam, the solution of M^T lam = dL/dx (solve(transpose=True)):
        SystemGradients(values, diag), each None unless asked for with True or with a tensor to write into.
          values: (nop, total) in the operator's layout: at every live entry of row j, in plane o,
                  -sum_b (sum_a coupling[a, b, o] lam[j, a]) x[col, b] (a per-point table: coupling[a, b, o, j], row j's own), and +0.0 in
                  the padding: dL/d(the entries of the value planes);
                  op._unpack's layout per slot through differentiable_stencil_system_solve's `coefficients`.
          diag:   (m, m, npoints), -(lam[i, a] * x[i, b]): dL/d(diag).
        One kernel launch on `stream` ("krylov-system-grads": one pass over the forward structure that reads the columns and writes the
        planes, never the values); no synchronisation, no allocation when the outputs are given.  lam and x are (npoints, m) as every
        vector of the solver; the outputs are contiguous float64 tensors on the operator's device that overlap neither lam, x, each
        other, the operator's values, the diag tensor nor the workspace."""
        import torch
        m = self._live()
        total = int(m["total"])
        asked = lambda flag: flag is not None and flag is not False
        if not (asked(values) or asked(diag)):
            raise ValueError("gradients: neither values nor diag is asked for")
        f64 = dict(dtype=torch.float64, device=self._device)
        with _torch_stream(stream, self._device):
            gval = torch.empty((self.nop, total), **f64) if values is True else (values if asked(values) else None)
            gdiag = torch.empty((self.m, self.m, self.npoints), **f64) if diag is True else (diag if asked(diag) else None)
        named = dict(lam=lam, x=x)
        self._vectors(**named)
        others = dict(named, workspace=self._ws, **{"the operator's values": self._op._val})
        if hasattr(self.diag, "dim"):
            others["diag"] = self.diag
        if self.per_point:
            others["coupling"] = self.coupling
        for t, name, shape, says in ((gval, "values", (self.nop, total), "the operator's layout"),
                                     (gdiag, "diag", (self.m, self.m, self.npoints), "the diag tensor's")):
            if t is None:
                continue
            if not hasattr(t, "dim") or not hasattr(t, "is_cuda"):
                raise ValueError("argument %s must be True, False or a device (HIP) tensor" % name)
            _check(t, name, "float64", len(shape))
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError("%s must be a contiguous float64 device tensor of shape %s, %s; got shape %s with strides %s"
                                 % (name, shape, says, tuple(t.shape), tuple(t.stride())))
            _same_device(self._ws, t)
            for other, held in others.items():
                if _overlap(t, held):
                    raise ValueError("%s overlaps %s in memory" % ("grad_diag" if name == "diag" else name, other))
            others["grad_diag" if name == "diag" else name] = t
        s, dev = _stream_and_device(x, stream)
        fn = B.lib().wlsqm_hip_krylov_system_point_grads_device if self.per_point else B.lib().wlsqm_hip_krylov_system_grads_device
        B.check(fn(
            m["nrows"], int(m["width"].shape[0]), _ptr(m["len"]), _ptr(m["width"]), _ptr(m["soff"]), _ptr(m["col"]), total, self.nop, self.m,
            _ptr(self.coupling) if self.per_point else C.cast(self._cp, C.c_void_p), _ptr(lam), _ptr(x),
            _ptr(gval) if gval is not None and total else None, _ptr(gdiag), dev, s))
        return SystemGradients(gval, gdiag)

    def coupling_gradient(self, lam, x, stream=None):
        """dL/d(coupling), a new device tensor (m, m, nop): entry (a, b, o) is -sum_i lam[i, a] (A_o x[:, b])_i.  No kernel of its own:
        the operator's stacked product on the m columns of x (op.apply, all planes in one pass) and a contraction with lam by torch, on
        `stream`: m elementwise products and sums over the points (a matrix product with one dimension of npoints is not what the
        BLAS behind torch.einsum is built for: 30 to 100 ms at 10^6 points, against about 1 ms).  It allocates its result and the
        products.  A per-point solver: (m, m, nop, npoints), entry (a, b, o, i) is -(lam[i, a] * (A_o x[:, b])_i), the same stacked
        product and one elementwise product, with no sum over the points."""
        import torch
        self._vectors(lam=lam, x=x)
        Y = self._op.apply(x.t(), stream=stream)                          # (m, nop, npoints): Y[b, o] = A_o x[:, b]
        with _torch_stream(stream, self._device):
            if self.per_point:
                return -(lam.t().contiguous()[:, None, None, :] * Y[None])   # contiguous, as the coupling tensor it is the gradient of
            return -torch.stack([(Y * lam[:, a]).sum(dim=-1) for a in range(self.m)])


def differentiable_stencil_solve(solver, b, x0=None, S=None, coefficients=None, rtol=1e-10, atol=0.0, maxiter=1000, check_every=8,
                                 adjoint_rtol=None, stream=None):
    """x (npoints,), the solution of M x = b by solver.solve, as a differentiable function of b, of solver.diag when that is a tensor,
    and of what the operator is made from: a new tensor with a grad_fn.

    S: the point table.  The forward runs solver's op.update(S.detach()) first (the operator must come from a fit, RuntimeError
    otherwise), and S receives dL/dS at fixed neighbour lists, with S's full shape.  coefficients=(slots, own): as
    StencilOperator.set_coefficients takes them (own None for an operator without own entries); the forward writes them into the
    operator first, and they receive the gradients of value plane `o`'s entries, exact zeros in the other planes and in the padding.
    Both given: ValueError.  With neither, the operator is not an input, and the backward pass reads it as it is then: an op.update
    or set_coefficients between forward and backward invalidates the graph, as any in-place change of a saved tensor does (it is not
    detected).  With either, the backward pass first puts the operator back where the forward had it (op.update(S, check=False), or
    set_coefficients), so that the steps of a time loop may share one operator and one solver.

    The forward solves from x0 (default zeros; it receives no gradient) to rtol / atol within maxiter iterations; a status other than
    0 is a RuntimeError that quotes the SolveInfo, and solver.info() afterwards is the forward's.  The backward pass solves
    M^T lam = dL/dx from zero (solve(transpose=True), relative tolerance `adjoint_rtol or rtol`; atol belongs to the forward alone;
    RuntimeError when it does not converge), then: b gets lam; diag and the coefficients get StencilSolver.gradients; S gets
    fit_cloud_geometry_adjoint_device on the fit of F = x with g_j = -scale * lam_j * rows[o].  Only what requires a gradient is
    computed, and nothing is launched when nothing does.  These are the gradients of the exact solution map (the implicit function
    theorem), accurate to the residuals of the two solves, not the derivative of the iteration.  `scale` is a Python float of the
    solver: its gradient is solver.gradients(lam, x, scale=True).  Not capturable: both passes read the solve's scalars on the host
    (RuntimeError inside a graph capture).  Once differentiable."""
    if not isinstance(solver, StencilSolver):
        raise ValueError("solver must be a StencilSolver")
    solver._live()
    op = solver._op
    if S is not None and coefficients is not None:
        raise ValueError("S and coefficients are two ways to make the operator: pass one of them")
    slots = own = None
    if coefficients is not None:
        if not isinstance(coefficients, (tuple, list)) or len(coefficients) != 2:
            raise ValueError("coefficients must be (slots, own), own None for an operator without own entries")
        slots, own = coefficients
        if slots is None:
            raise ValueError("coefficients must be (slots, own), own None for an operator without own entries")
    if S is not None and getattr(op, "_geo", None) is None:
        raise RuntimeError("the stencil operator was made from coefficients: there is no fit to redo")
    named = dict(b=b) if x0 is None else dict(b=b, x0=x0)
    solver._vectors(**named)                         # before anything is detached or cloned
    solver._tolerances(rtol, atol, maxiter)
    if adjoint_rtol is not None:
        solver._tolerances(adjoint_rtol, atol, maxiter)
    if int(check_every) < 1:
        raise ValueError("check_every must be >= 1; got %d" % int(check_every))
    solver._no_capture("differentiable_stencil_solve", stream)
    diag = solver.diag if hasattr(solver.diag, "dim") else None
    return _autograd().StencilSolve.apply(b, diag, S, slots, own, x0, solver, float(rtol), float(atol), int(maxiter), int(check_every),
                                          None if adjoint_rtol is None else float(adjoint_rtol), stream)


def differentiable_stencil_solve_many(solver, b, x0=None, rtol=1e-10, atol=0.0, maxiter=1000, check_every=8, adjoint_rtol=None, stream=None):
    """x (nfields, npoints), row f the solution of M x_f = b_f by solver.solve_many, as a differentiable function of b: a new tensor
    with a grad_fn.  The forward solves from x0 (default zeros; no gradient) and raises RuntimeError unless
    every field converges; the backward pass is ONE solve_many(transpose=True) from zero on the incoming gradient (relative tolerance
    `adjoint_rtol or rtol`, atol 0), and b gets its solution: row f of dL/db is, bit for bit, what differentiable_stencil_solve gives
    for field f alone.  With respect to b only: the gradients to the operator (S, coefficients), diag and scale of stacked solves are
    out of scope, and a diag tensor that requires a gradient gets none here.  Not capturable; once differentiable."""
    if not isinstance(solver, StencilSolver):
        raise ValueError("solver must be a StencilSolver")
    named = dict(b=b) if x0 is None else dict(b=b, x0=x0)
    solver._fields(**named)                          # before anything is detached or cloned
    solver._tolerances(rtol, atol, maxiter)
    if adjoint_rtol is not None:
        solver._tolerances(adjoint_rtol, atol, maxiter)
    if int(check_every) < 1:
        raise ValueError("check_every must be >= 1; got %d" % int(check_every))
    solver._no_capture("differentiable_stencil_solve_many", stream)
    return _autograd().StencilSolveMany.apply(b, x0, solver, float(rtol), float(atol), int(maxiter), int(check_every),
                                              None if adjoint_rtol is None else float(adjoint_rtol), stream)


def differentiable_stencil_system_solve(solver, b, x0=None, S=None, coefficients=None, coupling=None, rtol=1e-10, atol=0.0, maxiter=1000,
                                        check_every=8, adjoint_rtol=None, stream=None):
    """x (npoints, m), the solution of the coupled M x = b by solver.solve (a StencilSystemSolver), as a differentiable function of b,
    of solver.diag when that is a tensor, of `coupling` and of what the operator is made from: differentiable_stencil_solve's contract
    carried over to m fields.

    S: the point table; the forward runs op.update(S.detach()) first (RuntimeError for an operator without a fit), and S receives dL/dS
    at fixed neighbour lists.  coefficients=(slots, own) as StencilOperator.set_coefficients takes them, all nop planes: written into
    the operator first, and they receive the gradients of every plane's entries, exact zeros in the padding.  Both: ValueError.
    coupling: a float64 torch tensor (m, m, nop), on the host or on the device; the forward writes it into the solver
    (solver.set_coupling), and it receives its gradient on its own device.  For a solver with a per-point coupling it is the contiguous
    float64 device tensor (m, m, nop, npoints) that set_coupling takes, and its gradient has that shape: a coefficient field (DESIGN.md
    section 26).  Without it the solver's table is read as it is, in both passes.  With S, coefficients or coupling the backward pass first puts the operator and the table back where the forward had them,
    so that the steps of a loop may share one operator and one solver.

    The forward solves from x0 (default zeros; no gradient) to rtol / atol within maxiter iterations; a status other than 0 is a
    RuntimeError that quotes the SolveInfo.  The backward pass solves M^T lam = dL/dx from zero (solve(transpose=True), relative
    tolerance `adjoint_rtol or rtol`, atol 0; RuntimeError when it does not converge), then: b gets lam; diag and the coefficients get
    StencilSystemSolver.gradients; coupling gets coupling_gradient; S gets the geometry adjoint of the fits of F = x[:, b], summed over
    the components.  Only what requires a gradient is computed, and nothing is launched when nothing does.  Not capturable (RuntimeError
    inside a graph capture).  Once differentiable."""
    if not isinstance(solver, StencilSystemSolver):
        raise ValueError("solver must be a StencilSystemSolver")
    solver._live()
    op = solver._op
    if S is not None and coefficients is not None:
        raise ValueError("S and coefficients are two ways to make the operator: pass one of them")
    slots = own = None
    if coefficients is not None:
        if not isinstance(coefficients, (tuple, list)) or len(coefficients) != 2:
            raise ValueError("coefficients must be (slots, own), own None for an operator without own entries")
        slots, own = coefficients
        if slots is None:
            raise ValueError("coefficients must be (slots, own), own None for an operator without own entries")
    if S is not None and getattr(op, "_geo", None) is None:
        raise RuntimeError("the stencil operator was made from coefficients: there is no fit to redo")
    if coupling is not None:
        if not hasattr(coupling, "dim") or not hasattr(coupling, "is_cuda") or not hasattr(coupling, "requires_grad"):
            raise ValueError("coupling must be a float64 torch tensor (m, m, nop), on the host or on the device")
        if solver.per_point:
            solver._coupling_tensor(coupling, solver.nop, solver.npoints, solver._ws, solver.m)
        elif str(coupling.dtype) != "torch.float64" or tuple(coupling.shape) != (solver.m, solver.m, solver.nop):
            raise ValueError("coupling must be a float64 torch tensor of shape (%d, %d, %d); got %s of shape %s"
                             % (solver.m, solver.m, solver.nop, coupling.dtype, tuple(coupling.shape)))
    named = dict(b=b) if x0 is None else dict(b=b, x0=x0)
    solver._vectors(**named)                         # before anything is detached or cloned
    solver._tolerances(rtol, atol, maxiter)
    if adjoint_rtol is not None:
        solver._tolerances(adjoint_rtol, atol, maxiter)
    if int(check_every) < 1:
        raise ValueError("check_every must be >= 1; got %d" % int(check_every))
    solver._no_capture("differentiable_stencil_system_solve", stream)
    diag = solver.diag if hasattr(solver.diag, "dim") else None
    return _autograd().StencilSystemSolve.apply(b, diag, S, slots, own, coupling, x0, solver, float(rtol), float(atol), int(maxiter),
                                                int(check_every), None if adjoint_rtol is None else float(adjoint_rtol), stream)


# ---- batched dense solves (the kernels behind wlsqm.utils.lapackdrivers), device-resident ----

def _fortran3(A, name="A"):
    """A device float64 tensor (n, n, count) with the reference's Fortran layout: strides (1, n, n*n)."""
    _check(A, name, "float64", 3)
    n = int(A.shape[0])
    if int(A.shape[1]) != n or n < 1:
        raise ValueError("%s must have shape (n, n, count) with n >= 1, got %s" % (name, tuple(A.shape)))
    if A.shape[2] > 1 and A.stride() != (1, n, n * n) or A.shape[2] <= 1 and A.stride()[:2] != (1, n):
        raise ValueError("%s must be Fortran-ordered: strides (1, n, n*n), got %s" % (name, A.stride()))
    return n, int(A.shape[2])


def _fortran2(t, n, count, name, dtype_name):
    _check(t, name, dtype_name, 2)
    if tuple(t.shape) != (n, count):
        raise ValueError("%s must have shape (%d, %d), got %s" % (name, n, count, tuple(t.shape)))
    if count > 1 and t.stride() != (1, n) or count <= 1 and t.stride()[0] != 1:
        raise ValueError("%s must be Fortran-ordered: strides (1, %d), got %s" % (name, n, t.stride()))


def _same_device(ref, *ts):
    for t in ts:
        if t is not None and t.device != ref.device:
            raise ValueError("all tensors must be on the same device")


def _pivots_and_info(A, n, count, ipiv, info):
    import torch
    if ipiv is None:
        ipiv = torch.empty((count, n), dtype=torch.int32, device=A.device).t()
    _fortran2(ipiv, n, count, "ipiv", "int32")
    if info is None:
        info = torch.empty((count,), dtype=torch.int32, device=A.device)
    _check(info, "info", "int32", 1)
    if int(info.shape[0]) != count or (count > 1 and info.stride()[0] != 1):
        raise ValueError("info must be a contiguous (count,) int32 tensor")
    _same_device(A, ipiv, info)
    return ipiv, info


def _factor_batched(op, A, ipiv, info, stream):
    n, count = _fortran3(A)
    ipiv, info = _pivots_and_info(A, n, count, ipiv, info)
    s, dev = _stream_and_device(A, stream)
    B.check(getattr(B.lib(), "wlsqm_hip_%s_batched_device" % op)(n, count, _ptr(A), _ptr(ipiv), _ptr(info), dev, s))
    return ipiv, info


def _factor_solve_batched(op, A, b, ipiv, info, stream):
    n, count = _fortran3(A)
    _fortran2(b, n, count, "b", "float64")
    ipiv, info = _pivots_and_info(A, n, count, ipiv, info)
    _same_device(A, b)
    s, dev = _stream_and_device(A, stream)
    B.check(getattr(B.lib(), "wlsqm_hip_%s_batched_device" % op)(n, count, _ptr(A), _ptr(ipiv), _ptr(info), _ptr(b), dev, s))
    return ipiv, info


def _solve_batched(op, A, ipiv, b, stream):
    n, nlhs = _fortran3(A)
    _check(b, "b", "float64", 2)
    count = int(b.shape[1])
    if nlhs not in (1, count):
        raise ValueError("A holds %d factors: 1 (one factor for every right-hand side) or one per column of b (%d)" % (nlhs, count))
    _fortran2(b, n, count, "b", "float64")
    _fortran2(ipiv, n, nlhs, "ipiv", "int32")
    _same_device(A, ipiv, b)
    lhs_stride = 1 if nlhs == count and count > 1 else 0
    s, dev = _stream_and_device(A, stream)
    B.check(getattr(B.lib(), "wlsqm_hip_%s_batched_device" % op)(n, count, lhs_stride, _ptr(A), _ptr(ipiv), _ptr(b), dev, s))
    return b


def getrf_batched(A, ipiv=None, info=None, stream=None):
    """LU factorization with partial pivoting (dgetf2 semantics) of every matrix of the device tensor A (n, n, count),
    float64 with Fortran strides (1, n, n*n), in place on `stream` (default: the current stream).  Returns (ipiv, info):
    int32 (n, count) Fortran-ordered 1-based pivots and (count,) LAPACK INFO (j > 0: U(j, j) is exactly zero); both are
    allocated when not passed in."""
    return _factor_batched("getrf", A, ipiv, info, stream)


def getrs_batched(A, ipiv, b, stream=None):
    """Solve with the factors of getrf_batched: b (n, count) float64, Fortran-ordered, is overwritten by the solutions.
    A (n, n, count) / ipiv (n, count) give one factor per right-hand side; A (n, n, 1) / ipiv (n, 1) one factor for all
    of them.  Returns b."""
    return _solve_batched("getrs", A, ipiv, b, stream)


def gesv_batched(A, b, ipiv=None, info=None, stream=None):
    """getrf_batched + getrs_batched in one launch, one right-hand side per matrix: A gets the LU factors, b (n, count)
    the solutions.  As dgesv, a system whose info is > 0 (singular) is not solved: its column of b is left bit-unchanged,
    while its factor, pivots and info are written.  Returns (ipiv, info)."""
    return _factor_solve_batched("gesv", A, b, ipiv, info, stream)


def sytrf_batched(A, ipiv=None, info=None, stream=None):
    """Bunch-Kaufman U*D*U^T factorization (dsytf2 semantics, uplo='U') of the upper triangle of every matrix of A
    (n, n, count), in place; the strict lower triangle is neither read nor written.  Returns (ipiv, info) with dsytrf's
    pivot encoding."""
    return _factor_batched("sytrf", A, ipiv, info, stream)


def sytrs_batched(A, ipiv, b, stream=None):
    """Solve with the factors of sytrf_batched (one factor per right-hand side, or A (n, n, 1) for all).  Returns b."""
    return _solve_batched("sytrs", A, ipiv, b, stream)


def sysv_batched(A, b, ipiv=None, info=None, stream=None):
    """sytrf_batched + sytrs_batched in one launch, one right-hand side per matrix.  As dsysv, a system whose info is
    > 0 (singular D) is not solved: its column of b is left bit-unchanged.  Returns (ipiv, info)."""
    return _factor_solve_batched("sysv", A, b, ipiv, info, stream)


def symmetrize_batched(A, stream=None):
    """A[:, :, k] <- (A[:, :, k] + A[:, :, k]^T) / 2 for every k, in place.  Returns A."""
    n, count = _fortran3(A)
    s, dev = _stream_and_device(A, stream)
    B.check(B.lib().wlsqm_hip_symmetrize_batched_device(n, count, _ptr(A), dev, s))
    return A
