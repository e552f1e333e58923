"""ctypes binding of libwlsqm_hip.so (C ABI declared in include/wlsqm_hip.h).

There is no CPU fallback: if the shared library is missing the import of any fitting
entry point fails loudly, and if no HIP device is present the library itself returns
WLSQM_ENODEVICE (raised here as RuntimeError).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_lib", "libwlsqm_hip.so")

WLSQM_OK, WLSQM_EVALUE, WLSQM_ERUNTIME, WLSQM_EMEMORY, WLSQM_ENODEVICE = 0, -1, -2, -3, -4


class Batch(C.Structure):
    """struct wlsqm_batch (include/wlsqm_hip.h)."""
    _fields_ = [
        ("dimension", C.c_int32), ("do_sens", C.c_int32), ("ncases", C.c_int64),
        ("xk", C.c_void_p), ("xk_stride_case", C.c_int64), ("xk_stride_k", C.c_int64),
        ("fk", C.c_void_p), ("fk_stride_case", C.c_int64), ("fk_stride_k", C.c_int64),
        ("nk", C.c_void_p), ("nk_stride", C.c_int64),
        ("xi", C.c_void_p), ("xi_stride_case", C.c_int64),
        ("fi", C.c_void_p), ("fi_stride_case", C.c_int64),
        ("sens", C.c_void_p), ("sens_stride_case", C.c_int64), ("sens_stride_k", C.c_int64),
        ("order", C.c_void_p), ("order_stride", C.c_int64),
        ("knowns", C.c_void_p), ("knowns_stride", C.c_int64),
        ("weighting_method", C.c_void_p), ("wm_stride", C.c_int64),
        ("iterative", C.c_int32), ("max_iter", C.c_int32), ("max_nk", C.c_int64),
    ]


_lib = None


def _init_torch_hip_first():
    """PyTorch-ROCm wheels bundle their own HIP runtime (torch/lib/libamdhip64.so, no SONAME) next to the
    system one this library links (libamdhip64.so.7).  Both can live in one process, but only if torch's is
    initialised FIRST (the other order makes torch report "No HIP GPUs are available").  torch is the designated
    owner of device memory and streams for the device-resident API, so when it is installed we let it
    initialise the GPU before libwlsqm_hip.so is loaded.  Set WLSQM_HIP_SKIP_TORCH_INIT=1 to skip."""
    if os.environ.get("WLSQM_HIP_SKIP_TORCH_INIT") == "1":
        return
    try:
        import torch
    except Exception:
        return
    try:
        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:
        pass


def lib():
    """Load libwlsqm_hip.so; raises ImportError with build instructions if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "wlsqm: the HIP library %s is missing. Build it with python-wlsqm_amd/build.sh "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    _init_torch_hip_first()
    L = C.CDLL(LIB_PATH)
    L.wlsqm_hip_last_error.restype = C.c_char_p
    L.wlsqm_hip_last_kernel.restype = C.c_char_p
    L.wlsqm_hip_device_count.restype = C.c_int
    L.wlsqm_hip_number_of_dofs.argtypes = [C.c_int, C.c_int]
    L.wlsqm_hip_number_of_reduced_dofs.argtypes = [C.c_int, C.c_int64]
    L.wlsqm_hip_remap.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64]
    L.wlsqm_hip_fit_many_host.argtypes = [C.POINTER(Batch), C.c_int, C.POINTER(C.c_int32)]
    L.wlsqm_hip_fit_many_device.argtypes = [C.POINTER(Batch), C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                            C.c_int64, C.POINTER(C.c_int32)]
    L.wlsqm_hip_fit_many_device_orders.argtypes = [C.POINTER(Batch), C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_int32)]
    L.wlsqm_hip_fit_many_device_orders.restype = C.c_int
    L.wlsqm_hip_set_strict.argtypes = [C.c_int]
    L.wlsqm_hip_set_strict.restype = C.c_int
    L.wlsqm_hip_get_strict.restype = C.c_int
    if hasattr(L, "wlsqm_hip_set_row_hint"):                         # (tools/ab_lib.sh times older builds of the library through this binding)
        L.wlsqm_hip_set_row_hint.argtypes = [C.c_int]
        L.wlsqm_hip_set_row_hint.restype = C.c_int
        L.wlsqm_hip_set_order_hint.argtypes = [C.c_int]
        L.wlsqm_hip_set_order_hint.restype = C.c_int
    L.wlsqm_hip_strict_intermediates_device.argtypes = [C.POINTER(Batch), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                                        C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_int64]
    L.wlsqm_hip_strict_intermediates_device.restype = C.c_int
    L.wlsqm_hip_time_fit_device.argtypes = [C.POINTER(Batch), C.c_int, C.c_void_p, C.c_int, C.c_int,
                                            C.POINTER(C.c_float)]
    cloud = [C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
             C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    L.wlsqm_hip_fit_cloud_device.argtypes = cloud + [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                                     C.c_void_p, C.POINTER(C.c_int32)]
    L.wlsqm_hip_time_fit_cloud_device.argtypes = cloud + [C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_float)]
    # the adjoint of the fit (wlsqm.hip.fit_many_adjoint_device, fit_cloud_adjoint_device, differentiable_fit_*)
    L.wlsqm_hip_fit_adjoint_device.argtypes = [C.POINTER(Batch), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                               C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
    L.wlsqm_hip_fit_adjoint_device.restype = C.c_int
    L.wlsqm_hip_fit_cloud_adjoint_device.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                     C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    L.wlsqm_hip_fit_cloud_adjoint_device.restype = C.c_int
    # the geometry adjoint of the fit (wlsqm.hip.fit_many_geometry_adjoint_device, fit_cloud_geometry_adjoint_device)
    L.wlsqm_hip_fit_geometry_adjoint_device.argtypes = [C.POINTER(Batch), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                                        C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                                                        C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64]
    L.wlsqm_hip_fit_geometry_adjoint_device.restype = C.c_int
    L.wlsqm_hip_fit_cloud_geometry_adjoint_device.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                              C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                              C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                                              C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    L.wlsqm_hip_fit_cloud_geometry_adjoint_device.restype = C.c_int
    L.wlsqm_hip_expert_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.wlsqm_hip_knn_device.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.wlsqm_hip_knn_subset_device.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]
    L.wlsqm_hip_ball_device.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_void_p]
    L.wlsqm_hip_nearest_device.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int,
                                           C.c_void_p]
    if hasattr(L, "wlsqm_hip_grid_shape_host"):                      # (older builds of the library, as above)
        L.wlsqm_hip_grid_shape_host.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.wlsqm_hip_grid_shape_host.restype = C.c_int
    # the Morton order of a cloud and the renumbering of neighbour lists (csrc/order.hip)
    L.wlsqm_hip_spatial_order_device.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                 C.c_void_p]
    L.wlsqm_hip_spatial_keys_device.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.wlsqm_hip_relabel_hoods_device.argtypes = [C.c_int64, C.c_int, C.c_void_p, C.c_int64] + [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 3 \
        + [C.c_int, C.c_void_p]
    for name in ("spatial_order", "spatial_keys", "relabel_hoods"):
        getattr(L, "wlsqm_hip_%s_device" % name).restype = C.c_int
    L.wlsqm_hip_expert_interpolate_nearest.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p,
                                                       C.c_void_p]
    L.wlsqm_hip_expert_interpolate_continuous.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_int,
                                                          C.c_void_p]
    L.wlsqm_hip_expert_create_guest.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.wlsqm_hip_expert_prepare.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64]
    L.wlsqm_hip_expert_prepare_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64]
    L.wlsqm_hip_expert_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                                         C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_int32)]
    L.wlsqm_hip_expert_solve_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
    L.wlsqm_hip_expert_prepare_operator.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.wlsqm_hip_expert_solve_many_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64,
                                                     C.c_void_p, C.c_int64, C.c_int64]
    if hasattr(L, "wlsqm_hip_expert_solve_adjoint_device"):          # (older builds of the library, as above)
        L.wlsqm_hip_expert_solve_adjoint_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64,
                                                            C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64]
        L.wlsqm_hip_expert_solve_adjoint_device.restype = C.c_int
    L.wlsqm_hip_expert_solve_many.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                              C.c_void_p, C.c_int64, C.c_int64]
    L.wlsqm_hip_expert_memory_used.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.wlsqm_hip_expert_destroy.argtypes = [C.c_void_p]
    L.wlsqm_hip_expert_conds.argtypes = [C.c_void_p, C.c_void_p]
    L.wlsqm_hip_expert_interpolate.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_double, C.c_int, C.c_void_p]
    L.wlsqm_hip_interpolate_fit_host.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                                 C.c_int64, C.c_int, C.c_void_p, C.c_int]
    # interpolation plans (wlsqm.hip.InterpolationPlan, ExpertSolver.interpolation_plan)
    if hasattr(L, "wlsqm_hip_interp_plan_create"):                   # (older builds of the library, as above)
        L.wlsqm_hip_interp_plan_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64,
                                                   C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_void_p]
        L.wlsqm_hip_interp_plan_create_expert.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                                          C.c_int64, C.c_double, C.c_void_p]
        L.wlsqm_hip_interp_plan_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_int64)] * 4
        L.wlsqm_hip_interp_plan_export.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.wlsqm_hip_interp_plan_eval_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64,
                                                        C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_int64, C.c_int64]
        L.wlsqm_hip_interp_plan_eval_expert.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_void_p,
                                                        C.c_int64]
        L.wlsqm_hip_interp_plan_destroy.argtypes = [C.c_void_p]
        for name in ("create", "create_expert", "info", "export", "eval_device", "eval_expert", "destroy"):
            getattr(L, "wlsqm_hip_interp_plan_" + name).restype = C.c_int
        # the adjoint of the evaluation (InterpolationPlan.evaluate_adjoint, wlsqm.hip.differentiable_evaluate)
        L.wlsqm_hip_interp_plan_prepare_adjoint.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        L.wlsqm_hip_interp_plan_adjoint_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_int64)] * 3 + [C.POINTER(C.c_int32)]
        L.wlsqm_hip_interp_plan_export_transposed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.wlsqm_hip_interp_plan_eval_adjoint_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.c_int,
                                                                C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64,
                                                                C.c_int]
        for name in ("prepare_adjoint", "adjoint_info", "export_transposed", "eval_adjoint_device"):
            getattr(L, "wlsqm_hip_interp_plan_" + name).restype = C.c_int
    # stencil operators (wlsqm.hip.StencilOperator): the SELL-64 product
    if hasattr(L, "wlsqm_hip_sell_apply_device"):                    # (older builds of the library, as above)
        L.wlsqm_hip_sell_apply_device.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                                  C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_int, C.c_void_p]
        L.wlsqm_hip_sell_apply_device.restype = C.c_int
    # the fused build of the value planes on a moved cloud and the transposed values (StencilOperator.update)
    if hasattr(L, "wlsqm_hip_stencil_build_device"):
        L.wlsqm_hip_stencil_build_device.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                     C.c_int64, C.c_int, C.c_void_p]
        L.wlsqm_hip_stencil_build_device.restype = C.c_int
        L.wlsqm_hip_sell_permute_device.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int,
                                                    C.c_int, C.c_void_p]
        L.wlsqm_hip_sell_permute_device.restype = C.c_int
    # implicit solves with a stencil operator (wlsqm.hip.StencilSolver): BiCGSTAB resident on the device
    if hasattr(L, "wlsqm_hip_krylov_start_device"):                  # (older builds of the library, as above)
        system = [C.c_int64, C.c_int64] + [C.c_void_p] * 6 + [C.c_double, C.c_double]     # the SELL-64 arrays, diag, diag_const, scale
        L.wlsqm_hip_krylov_workspace_bytes.argtypes = [C.c_int64]
        L.wlsqm_hip_krylov_workspace_bytes.restype = C.c_int64
        L.wlsqm_hip_krylov_start_device.argtypes = system + [C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int64, C.c_void_p,
                                                             C.c_int, C.c_void_p]
        L.wlsqm_hip_krylov_bicgstab_device.argtypes = system + [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]
        L.wlsqm_hip_krylov_product_device.argtypes = system + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        for name in ("start", "bicgstab", "product"):
            getattr(L, "wlsqm_hip_krylov_%s_device" % name).restype = C.c_int
    # the gradients through such a solve (StencilSolver.gradients)
    if hasattr(L, "wlsqm_hip_krylov_grads_device"):
        L.wlsqm_hip_krylov_grads_device.argtypes = ([C.c_int64, C.c_int64] + [C.c_void_p] * 6 + [C.c_double, C.c_double]
                                                    + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_int, C.c_void_p])
        L.wlsqm_hip_krylov_grads_device.restype = C.c_int
    # the block-Jacobi preconditioner of those solves (wlsqm.hip.BlockJacobi)
    if hasattr(L, "wlsqm_hip_krylov_block_factor_device"):
        system = [C.c_int64, C.c_int64] + [C.c_void_p] * 6 + [C.c_double, C.c_double]
        L.wlsqm_hip_krylov_block_bytes.argtypes = [C.c_int64, C.c_int]
        L.wlsqm_hip_krylov_block_bytes.restype = C.c_int64
        L.wlsqm_hip_krylov_block_factor_device.argtypes = system + [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.wlsqm_hip_krylov_block_start_device.argtypes = system + [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double,
                                                                   C.c_int64, C.c_void_p, C.c_int, C.c_void_p]
        L.wlsqm_hip_krylov_block_bicgstab_device.argtypes = system + [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int,
                                                                      C.c_void_p]
        L.wlsqm_hip_krylov_block_precondition_device.argtypes = [C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        for name in ("factor", "start", "bicgstab", "precondition"):
            getattr(L, "wlsqm_hip_krylov_block_%s_device" % name).restype = C.c_int
    # stacked right-hand sides of those solves (StencilSolver(nfields=...).solve_many)
    if hasattr(L, "wlsqm_hip_krylov_many_start_device"):
        system = [C.c_int64, C.c_int64] + [C.c_void_p] * 6 + [C.c_double, C.c_double]
        fields = [C.c_void_p, C.c_int64, C.c_int64]                    # a (nfields, nrows) array, its field and point strides
        L.wlsqm_hip_krylov_many_workspace_bytes.argtypes = [C.c_int64, C.c_int]
        L.wlsqm_hip_krylov_many_workspace_bytes.restype = C.c_int64
        L.wlsqm_hip_krylov_many_start_device.argtypes = (system + [C.c_int] + fields + fields + [C.c_int, C.c_void_p, C.c_double, C.c_double,
                                                                                                 C.c_int64, C.c_void_p, C.c_int, C.c_void_p])
        L.wlsqm_hip_krylov_many_bicgstab_device.argtypes = system + [C.c_int] + fields + [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int,
                                                                                           C.c_void_p]
        L.wlsqm_hip_krylov_many_product_device.argtypes = system + [C.c_int] + fields * 3 + [C.c_void_p, C.c_int, C.c_void_p]
        for name in ("start", "bicgstab", "product"):
            getattr(L, "wlsqm_hip_krylov_many_%s_device" % name).restype = C.c_int
    # BiCGSTAB(2) on those systems (StencilSolver(method="bicgstab2"))
    if hasattr(L, "wlsqm_hip_krylov_l2_start_device"):
        system = [C.c_int64, C.c_int64] + [C.c_void_p] * 6 + [C.c_double, C.c_double]
        L.wlsqm_hip_krylov_l2_workspace_bytes.argtypes = [C.c_int64]
        L.wlsqm_hip_krylov_l2_workspace_bytes.restype = C.c_int64
        L.wlsqm_hip_krylov_l2_start_device.argtypes = system + [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int64,
                                                                C.c_void_p, C.c_int, C.c_void_p]
        L.wlsqm_hip_krylov_l2_start_device.restype = C.c_int
        L.wlsqm_hip_krylov_l2_device.argtypes = system + [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]
        L.wlsqm_hip_krylov_l2_device.restype = C.c_int
    # the sparse approximate inverse preconditioner of those solves (wlsqm.hip.ApproximateInverse)
    if hasattr(L, "wlsqm_hip_krylov_spai_build_device"):
        system = [C.c_int64, C.c_int64] + [C.c_void_p] * 6 + [C.c_double, C.c_double]
        L.wlsqm_hip_krylov_spai_bytes.argtypes = [C.c_int64, C.c_int64]
        L.wlsqm_hip_krylov_spai_bytes.restype = C.c_int64
        L.wlsqm_hip_krylov_spai_build_device.argtypes = system + [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                                  C.c_void_p]
        L.wlsqm_hip_krylov_spai_apply_device.argtypes = [C.c_int64, C.c_int64] + [C.c_void_p] * 7 + [C.c_int, C.c_void_p]
        L.wlsqm_hip_krylov_spai_start_device.argtypes = system + [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int64,
                                                                  C.c_void_p, C.c_int, C.c_void_p]
        L.wlsqm_hip_krylov_spai_iterate_device.argtypes = system + [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]
        for name in ("build", "apply", "start", "iterate"):
            getattr(L, "wlsqm_hip_krylov_spai_%s_device" % name).restype = C.c_int
    # the overlapping blocks of those solves (wlsqm.hip.OverlappingBlocks)
    if hasattr(L, "wlsqm_hip_krylov_schwarz_build_device"):
        system = [C.c_int64, C.c_int64] + [C.c_void_p] * 6 + [C.c_double, C.c_double]
        sets = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]       # block, rows, table, planes
        L.wlsqm_hip_krylov_schwarz_bytes.argtypes = [C.c_int64, C.c_int, C.c_int]
        L.wlsqm_hip_krylov_schwarz_bytes.restype = C.c_int64
        L.wlsqm_hip_krylov_schwarz_build_device.argtypes = system + sets + [C.c_void_p, C.c_int, C.c_void_p]
        L.wlsqm_hip_krylov_schwarz_apply_device.argtypes = [C.c_int64] + sets + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.wlsqm_hip_krylov_schwarz_start_device.argtypes = system + [C.c_int] + sets + [C.c_void_p, C.c_void_p, C.c_double, C.c_double,
                                                                                      C.c_int64, C.c_void_p, C.c_int, C.c_void_p]
        L.wlsqm_hip_krylov_schwarz_iterate_device.argtypes = system + [C.c_int] + sets + [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]
        for name in ("build", "apply", "start", "iterate"):
            getattr(L, "wlsqm_hip_krylov_schwarz_%s_device" % name).restype = C.c_int
    # coupled fields on one cloud (wlsqm.hip.StencilSystemSolver)
    if hasattr(L, "wlsqm_hip_krylov_system_start_device"):
        # the SELL-64 arrays, total, nop, m, coupling (host), diag (device), diag_const (host)
        coupled = [C.c_int64, C.c_int64] + [C.c_void_p] * 5 + [C.c_int64, C.c_int, C.c_int] + [C.c_void_p] * 3
        L.wlsqm_hip_krylov_system_workspace_bytes.argtypes = [C.c_int64, C.c_int]
        L.wlsqm_hip_krylov_system_workspace_bytes.restype = C.c_int64
        L.wlsqm_hip_krylov_system_start_device.argtypes = coupled + [C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int64,
                                                                    C.c_void_p, C.c_int, C.c_void_p]
        L.wlsqm_hip_krylov_system_bicgstab_device.argtypes = coupled + [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]
        L.wlsqm_hip_krylov_system_product_device.argtypes = coupled + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        for name in ("start", "bicgstab", "product"):
            getattr(L, "wlsqm_hip_krylov_system_%s_device" % name).restype = C.c_int
    # their transposed forms and the gradients through such a solve (StencilSystemSolver.gradients)
    if hasattr(L, "wlsqm_hip_krylov_system_grads_device"):
        for name in ("start", "bicgstab", "product"):
            fn = getattr(L, "wlsqm_hip_krylov_system_%s_transposed_device" % name)
            fn.argtypes = getattr(L, "wlsqm_hip_krylov_system_%s_device" % name).argtypes
            fn.restype = C.c_int
        L.wlsqm_hip_krylov_system_grads_device.argtypes = ([C.c_int64, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_int, C.c_int]
                                                           + [C.c_void_p] * 5 + [C.c_int, C.c_void_p])
        L.wlsqm_hip_krylov_system_grads_device.restype = C.c_int
    # a per-point coupling: coupling is a device tensor, then transposed and the mixed plane (StencilSystemSolver)
    if hasattr(L, "wlsqm_hip_krylov_system_point_start_device"):
        point = coupled + [C.c_int, C.c_void_p]
        L.wlsqm_hip_krylov_system_point_start_device.argtypes = point + L.wlsqm_hip_krylov_system_start_device.argtypes[len(coupled):]
        L.wlsqm_hip_krylov_system_point_bicgstab_device.argtypes = point + L.wlsqm_hip_krylov_system_bicgstab_device.argtypes[len(coupled):]
        L.wlsqm_hip_krylov_system_point_product_device.argtypes = point + L.wlsqm_hip_krylov_system_product_device.argtypes[len(coupled):]
        L.wlsqm_hip_krylov_system_point_grads_device.argtypes = L.wlsqm_hip_krylov_system_grads_device.argtypes
        for name in ("start", "bicgstab", "product", "grads"):
            getattr(L, "wlsqm_hip_krylov_system_point_%s_device" % name).restype = C.c_int
    # block-Jacobi over points for coupled fields (wlsqm.hip.PointBlockJacobi): points, planes in jacobi's place
    if hasattr(L, "wlsqm_hip_krylov_system_block_factor_device"):
        point = coupled + [C.c_int, C.c_void_p]
        blocks = [C.c_int, C.c_void_p]
        L.wlsqm_hip_krylov_system_block_bytes.argtypes = [C.c_int64, C.c_int, C.c_int]
        L.wlsqm_hip_krylov_system_block_bytes.restype = C.c_int64
        L.wlsqm_hip_krylov_system_block_factor_device.argtypes = coupled + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.wlsqm_hip_krylov_system_block_gather_device.argtypes = coupled + [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.wlsqm_hip_krylov_system_block_precondition_device.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                                        C.c_void_p]
        start = L.wlsqm_hip_krylov_system_start_device.argtypes[len(coupled) + 1:]
        iterate = L.wlsqm_hip_krylov_system_bicgstab_device.argtypes[len(coupled) + 1:]
        for name in ("system_block_start", "system_block_start_transposed"):
            getattr(L, "wlsqm_hip_krylov_%s_device" % name).argtypes = coupled + blocks + start
        for name in ("system_block_bicgstab", "system_block_bicgstab_transposed"):
            getattr(L, "wlsqm_hip_krylov_%s_device" % name).argtypes = coupled + blocks + iterate
        L.wlsqm_hip_krylov_system_point_block_start_device.argtypes = point + blocks + start
        L.wlsqm_hip_krylov_system_point_block_bicgstab_device.argtypes = point + blocks + iterate
        for name in ("system_block_factor", "system_block_gather", "system_block_precondition", "system_block_start", "system_block_start_transposed",
                     "system_block_bicgstab", "system_block_bicgstab_transposed", "system_point_block_start", "system_point_block_bicgstab"):
            getattr(L, "wlsqm_hip_krylov_%s_device" % name).restype = C.c_int
    # batched dense solves (wlsqm.utils.lapackdrivers, wlsqm.hip.*_batched)
    for op in ("getrf", "gesv", "sytrf", "sysv"):
        solve = op in ("gesv", "sysv")
        rest = [C.c_void_p] * (4 if solve else 3)
        getattr(L, "wlsqm_hip_%s_batched_device" % op).argtypes = [C.c_int, C.c_int64] + rest + [C.c_int, C.c_void_p]
        getattr(L, "wlsqm_hip_%s_batched_host" % op).argtypes = [C.c_int, C.c_int64] + rest + [C.c_int]
    for op in ("getrs", "sytrs"):
        getattr(L, "wlsqm_hip_%s_batched_device" % op).argtypes = [C.c_int, C.c_int64, C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p]
        getattr(L, "wlsqm_hip_%s_batched_host" % op).argtypes = [C.c_int, C.c_int64, C.c_int] + [C.c_void_p] * 3 + [C.c_int]
    L.wlsqm_hip_symmetrize_batched_device.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]
    L.wlsqm_hip_symmetrize_batched_host.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.c_int]
    for op in ("getrf", "getrs", "gesv", "sytrf", "sytrs", "sysv", "symmetrize"):
        getattr(L, "wlsqm_hip_%s_batched_device" % op).restype = C.c_int
        getattr(L, "wlsqm_hip_%s_batched_host" % op).restype = C.c_int
    for name in ("wlsqm_hip_fit_many_host", "wlsqm_hip_fit_many_device", "wlsqm_hip_time_fit_device",
                 "wlsqm_hip_expert_create", "wlsqm_hip_expert_create_guest", "wlsqm_hip_expert_prepare", "wlsqm_hip_expert_prepare_device", "wlsqm_hip_expert_solve",
                 "wlsqm_hip_expert_solve_device", "wlsqm_hip_expert_prepare_operator", "wlsqm_hip_expert_solve_many_device", "wlsqm_hip_expert_solve_many",
                 "wlsqm_hip_expert_memory_used", "wlsqm_hip_expert_destroy",
                 "wlsqm_hip_expert_conds", "wlsqm_hip_expert_interpolate", "wlsqm_hip_interpolate_fit_host",
                 "wlsqm_hip_fit_cloud_device", "wlsqm_hip_time_fit_cloud_device", "wlsqm_hip_knn_device", "wlsqm_hip_knn_subset_device", "wlsqm_hip_ball_device", "wlsqm_hip_nearest_device",
                 "wlsqm_hip_expert_interpolate_nearest", "wlsqm_hip_expert_interpolate_continuous",
                 "wlsqm_hip_number_of_dofs", "wlsqm_hip_number_of_reduced_dofs", "wlsqm_hip_remap"):
        getattr(L, name).restype = C.c_int
    _lib = L
    return L


def check(rc):
    """Map a WLSQM_E* code to the exception class the reference raises (SURVEY §8b 'Errors')."""
    if rc == WLSQM_OK:
        return
    msg = lib().wlsqm_hip_last_error().decode("utf-8", "replace")
    if rc == WLSQM_EVALUE:
        raise ValueError(msg)
    if rc == WLSQM_EMEMORY:
        raise MemoryError(msg)
    raise RuntimeError(msg)


def default_device():
    """Device of the host-array entry points, in this order: WLSQM_HIP_DEVICE if set; torch's current device when torch has
    initialised the GPU in this process AND that device is not the default 0 (the caller said torch.cuda.set_device /
    torch.cuda.device); LOCAL_RANK when set (one process per GPU under torch.distributed.run: a rank that only ever named
    'cuda:<local_rank>' explicitly still has current_device() == 0) AND that ordinal exists — a launcher that isolates one GPU per
    rank (HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES) leaves every rank with device 0 only, and LOCAL_RANK = 3 names nothing there;
    otherwise torch's current device, otherwise 0."""
    if "WLSQM_HIP_DEVICE" in os.environ:
        return int(os.environ["WLSQM_HIP_DEVICE"])
    import sys
    torch = sys.modules.get("torch")
    cur = None
    if torch is not None:
        try:
            if torch.cuda.is_initialized():
                cur = int(torch.cuda.current_device())
        except Exception:
            cur = None
    if cur:
        return cur
    if "LOCAL_RANK" in os.environ:
        lr = int(os.environ["LOCAL_RANK"])
        try:
            ndev = int(lib().wlsqm_hip_device_count())
        except Exception:
            ndev = 0
        if 0 <= lr < ndev or ndev <= 0:                 # (no visible device at all: keep the rank's number, the call fails loudly anyway)
            return lr
    return cur or 0


# ---- argument coercion with the reference's typed-memoryview rules (SURVEY §8b 'Array typing') ----

def view(a, dtype, ndim, name, contiguous_last=False, writable=False):
    """np.ndarray view of `a` with Cython-memoryview-like checks: exact dtype, exact ndim, and
    (when the reference declares ::view.contiguous) unit stride on the last axis."""
    arr = np.asarray(a)
    if arr.dtype != np.dtype(dtype):
        raise ValueError("Buffer dtype mismatch, expected '%s' but got '%s' (argument %s)"
                         % (np.dtype(dtype).name, arr.dtype.name, name))
    if arr.ndim != ndim:
        raise ValueError("Buffer has wrong number of dimensions (expected %d, got %d) (argument %s)"
                         % (ndim, arr.ndim, name))
    if contiguous_last and arr.shape[-1] > 1 and arr.strides[-1] != arr.itemsize:
        raise ValueError("Buffer and memoryview are not contiguous in the same dimension. (argument %s)" % name)
    if any(s % arr.itemsize for s in arr.strides):
        raise ValueError("argument %s: strides must be multiples of the item size" % name)
    if writable and not arr.flags.writeable:
        raise ValueError("buffer source array is read-only (argument %s)" % name)
    return arr


def es(arr, axis):
    """element stride"""
    return arr.strides[axis] // arr.itemsize
