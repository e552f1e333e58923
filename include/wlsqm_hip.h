/* wlsqm_hip.h — C ABI of libwlsqm_hip.so, the MI355X (gfx950) batched WLSQM fitter.
 *
 * This is the drop-in boundary for ONE hot path of Technologicat/python-wlsqm:
 * the per-case "assemble weighted normal equations -> factor -> solve" loop behind
 * wlsqm.fitter.simple.fit_*D_many[_parallel] / fit_*D_iterative_many[_parallel]
 * and wlsqm.fitter.expert.ExpertSolver.prepare()/solve().  The reference has no
 * FFI layer of its own (it is Cython); each entry point below names the reference
 * interface it replaces (file:line relative to the reference repo).  Plain pointers
 * and sizes only; no torch / numpy types.  All functions return 0 on success or a
 * negative WLSQM_E* code; wlsqm_hip_last_error() gives a thread-local message.
 *
 * Strides are in ELEMENTS of the array's dtype (not bytes).  Arrays follow the
 * reference's layout contract (simple.pyx:131-159): the innermost axis of xk, xi,
 * fi and sens must be contiguous, every other axis may have any stride.
 */
#ifndef WLSQM_HIP_H
#define WLSQM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- constants: wlsqm/fitter/defs.pyx:69-75 ---- */
#define WLSQM_ALGO_BASIC      1
#define WLSQM_ALGO_ITERATIVE  2
#define WLSQM_WEIGHT_UNIFORM  1
#define WLSQM_WEIGHT_CENTER   2

/* ---- error codes (mapped by the Python shim to the reference's exception classes) ---- */
#define WLSQM_OK            0
#define WLSQM_EVALUE       -1   /* -> ValueError   (bad dimension/order/length; expert.pyx:131-159, infra.pyx:311-313) */
#define WLSQM_ERUNTIME     -2   /* -> RuntimeError (solve before prepare, expert.pyx:493-494; HIP failure) */
#define WLSQM_EMEMORY      -3   /* -> MemoryError  (infra.pyx:237,243,363,819) */
#define WLSQM_ENODEVICE    -4   /* -> RuntimeError: no HIP device; there is NO CPU fallback in this library */

const char* wlsqm_hip_last_error(void);
/* Diagnostics: name of the kernel family the last fit launch of this thread dispatched to ("tile", "tile-gather",
 * "tile1", "tile1-extras", "tilek", "moment", "rows", "lane", "wave", "solve-many"; "" before the first launch).  The tests
 * use it to make sure a fast path is what they exercise. */
const char* wlsqm_hip_last_kernel(void);

/* Number of usable HIP devices (0 if none).  Never initialises a context on failure. */
int wlsqm_hip_device_count(void);

/* ---- host-side index contract (pure integer work, bit-exact with the reference) ---- */

/* infra.pyx:67-112  number_of_dofs: returns no, or -1 (bad dimension) / -2 (bad order). */
int wlsqm_hip_number_of_dofs(int dimension, int order);
/* infra.pyx:119-121 number_of_reduced_dofs = n - popcountll(mask) (bits >= n are NOT masked off). */
int wlsqm_hip_number_of_reduced_dofs(int n, int64_t mask);
/* infra.pyx:145-200 remap: fills o2r[n], r2o[n] with -1 sentinels, returns nr. */
int wlsqm_hip_remap(int32_t* o2r, int32_t* r2o, int n, int64_t mask);

/* ---- batch description shared by the fit entry points ----
 * Mirrors the argument list of simple.pyx:953-957 generic_fit_basic_many_parallel
 * (and :1065-1069 for the iterative variant).  dimension==1: xk is [ncases,max_nk]
 * (xk_stride_k is the neighbour stride), xi is [ncases].
 */
typedef struct wlsqm_batch {
    int32_t dimension;            /* 1, 2 or 3 */
    int32_t do_sens;              /* simple.pyx: do_sens */
    int64_t ncases;
    const double*  xk;   int64_t xk_stride_case, xk_stride_k;   /* [j,k,m], m contiguous */
    const double*  fk;   int64_t fk_stride_case, fk_stride_k;   /* [j,k] */
    const int32_t* nk;   int64_t nk_stride;                     /* [j] */
    const double*  xi;   int64_t xi_stride_case;                /* [j,m], m contiguous */
    double*        fi;   int64_t fi_stride_case;                /* [j,n] in/out: knowns read, unknowns written */
    double*        sens; int64_t sens_stride_case, sens_stride_k; /* [j,k,n] or NULL */
    const int32_t* order;            int64_t order_stride;      /* [j] */
    const int64_t* knowns;           int64_t knowns_stride;     /* [j] */
    const int32_t* weighting_method; int64_t wm_stride;         /* [j] */
    int32_t iterative;            /* 0: ALGO_BASIC body (impl.pyx:731 solve); 1: impl.pyx:986 solve_iterative */
    int32_t max_iter;             /* simple.pyx:112 default 10 */
    int64_t max_nk;               /* extent of the k axis of xk/fk/sens (upper bound on nk[j]) */
} wlsqm_batch;

/* fit_{1,2,3}D_many_parallel / _iterative_many_parallel on HOST arrays
 * (simple.pyx:192-234, 379-421, 562-604; drivers :953-1058, :1065-1170).
 * Copies the batch to the device, runs the HIP kernels, commits fi (and sens) back.
 * Aliasing guarantee of simple.pyx:1010-1019 holds: all inputs are read before any
 * output is committed.  *iterations_out (nullable) receives the return value of the
 * reference function: 0 for basic, max refinement iterations otherwise.
 * device: HIP device ordinal. */
int wlsqm_hip_fit_many_host(const wlsqm_batch* b, int device, int32_t* iterations_out);

/* Same computation on DEVICE-RESIDENT arrays (all pointers in `b` are device pointers of
 * `device`), enqueued on `stream` (a hipStream_t, NULL = default stream).  With iterations_out == NULL the
 * call only enqueues kernels (no allocation, no host synchronisation: it can be captured into a hipGraph, refinement
 * included); with iterations_out != NULL (a host pointer) and b->iterative it allocates a stream-ordered 4-byte counter,
 * copies it back and synchronises `stream`.  The arrays must cover b->ncases rows (or every row `case_index` names),
 * b->max_nk neighbour slots per row and number_of_dofs(dimension, order_uniform) columns of fi (and of sens); nk[j]
 * is clamped to b->max_nk by every kernel.
 * `order_uniform` >= 0 states that every case has this order (required: the kernels are
 * specialised per (dimension, order); heterogeneous batches are bucketed by the caller,
 * one call per order with `case_index`).  `case_index` (device, nullable): the ncases_sel
 * case numbers to process; NULL = all b->ncases cases in order.
 * fi is updated in place (knowns untouched); the caller guarantees fk/xk do not alias fi. */
int wlsqm_hip_fit_many_device(const wlsqm_batch* b, int device, void* stream, int order_uniform,
                              const int64_t* case_index, int64_t ncases_sel, int32_t* iterations_out);

/* Per-case polynomial orders on the device-resident path (the reference takes a per-case `order` array, simple.pyx:379-381):
 * as wlsqm_hip_fit_many_device, with order_dev[j * order_stride] (int32, DEVICE memory) instead of order_uniform.  The cases are
 * bucketed by order ON THE DEVICE (one counting kernel, index lists in stream-ordered scratch) and every bucket is launched
 * with its size left in device memory: no host synchronisation, nothing but kernel launches and stream-ordered allocations
 * unless iterations_out is given.  b->order is not read.  max_order (0..4) is the largest order the caller's fi / sens rows are
 * wide enough for (the reference's "(ncases, >= max no)" rule, simple.pyx:379-381): cases whose order is not 0..max_order are
 * left untouched and their buckets are never launched.  The buckets are STABLE (ascending case number: a stable counting
 * partition, no atomics on positions), so results are bit-identical from run to run. */
int wlsqm_hip_fit_many_device_orders(const wlsqm_batch* b, int device, void* stream, const int32_t* order_dev, int64_t order_stride,
                                     int max_order, int32_t* iterations_out);

/* ---- numerics mode (extension) ----
 * 0 (default): the fast kernels — moment form, neighbour sums split over lanes, FMA contraction, LDL^T: results agree with the
 *    reference to kappa * eps rounding.
 * 1: reference-order arithmetic (csrc/fit_strict.hip): every floating-point operation of make_c_nD / Case_make_weights / make_A
 *    (impl.pyx:70-602, infra.pyx:668-702), rescale_ruiz2001_c (lapackdrivers.pyx:553-623), dgetrf / dgetrs (:1628-1665), solve
 *    and solve_iterative (impl.pyx:731-1083) in the reference's order, one lane per case, IEEE divide and sqrt, no FMA contraction.
 *    Applies to every entry point that fits (wlsqm_hip_fit_many_*, wlsqm_hip_fit_cloud_device, wlsqm_hip_expert_solve*; a stacked
 *    solve runs one fit per field).  Several times slower; for validation against the reference at 1e-10.
 * 2: accurate (csrc/fit_accurate.hip): mode 1 with ONE change — the normal matrix of make_A (impl.pyx:566-602) is assembled from
 *    its upper triangle, entry (j, m) = sum_k (w c_m) c_j for m >= j, and mirrored; the equilibration then sees a symmetric matrix
 *    (row and column scales coincide bit for bit) and runs one pass per sweep.  Quotients and roots are correctly rounded (the
 *    compiler's IEEE sequences without their range scaling where every operand is checked to be in range, the full sequences
 *    otherwise).  Applies to the basic fits of the 2D / 3D systems up to 10 unknowns (2D orders 0-3, 3D orders 0-2) with EVERY
 *    knowns mask (stray bits beyond the polynomial's DOFs included), both weightings, dense, strided or index-based input and
 *    ragged neighbour counts; every other call of the mode (1D, 2D order 4, 3D orders 3-4, sensitivities, refinement) runs mode 1.  Within 1e-10 of the reference on every column of BASELINE
 *    configs[1] and configs[4] (as mode 1), at the fast kernels' order of magnitude in time.
 * 3: contracted (csrc/fit_accurate.hip, its FMA instantiations; wlsqm_hip_last_kernel: "accurate-fma"): mode 2 with a += b * c
 *    fused into one rounding in the neighbour sums of the matrix (acc = fma(w c_m, c_j, acc), the product w c_m rounded first)
 *    and of the right-hand side (acc = fma(w f_k, c_a, acc)), in the update of the LU's trailing matrix and in the forward and
 *    back substitution — and nowhere else: the monomials, the weights, the equilibration, the scaling, the term-by-term
 *    elimination of known DOFs, every quotient and the un-scaling are mode 2's.  Coverage and dispatch are mode 2's, as stated
 *    above: the same shapes, masks, weightings and input forms run the fused kernels, everything else runs mode 1.
 *    Still within 1e-10 of the reference on every column of configs[1] and configs[4], but with less room: 5.4e-11 and 5.3e-11
 *    on the 1M-point samples and 9.0e-11 on the 16M-point configs[4] sample (1 024 cases each) — a 10 % margin there, where
 *    mode 2 is at 2.3e-11.
 * The mode belongs to the calling thread; its initial value is the environment variable WLSQM_HIP_STRICT (unset / 0: fast; 1;
 * 2 or "accurate"; 3 or "contracted" — first character 2 / a / A and 3 / c / C; before mode 3 existed the latter three selected
 * mode 1, as every other value does).  wlsqm_hip_set_strict takes 0..3 (any other nonzero value: 1) and returns the previous
 * mode. */
int wlsqm_hip_set_strict(int mode);
int wlsqm_hip_get_strict(void);

/* Round 6: what the calling thread knows about the neighbour counts nk[j] of the DENSE DEVICE-RESIDENT batches it hands over (only
 * entries below nk[j] of a row are touched: simple.pyx:147; the reference's own harness passes ball-query rows of 100 slots with 30..100
 * valid entries, examples/wlsqm_example.py:103-133):
 *   1 (default) every case fills its row, or nearly: the plain kernels;
 *   2 ragged: the staged kernels run the copy whose waves move only the chunks their own 64 cases need (csrc/fit_stage.hip);
 *   0 unknown: the plain kernels mark the waves none of whose cases reaches the row's last chunk and the ragged copy runs those
 *     behind them (an idle launch, ~2 us, for a batch of full rows).
 * A hint, never a condition of correctness: every setting returns the same bits.  The host entry points (wlsqm_hip_fit_many_host)
 * look at the counts themselves and ignore it.  Returns the previous value. */
int wlsqm_hip_set_row_hint(int hint);

/* Round 6: are the neighbours of every row sorted by distance (1, the default: what a k-nearest-neighbour search returns — scipy's cKDTree.query,
 * wlsqm_hip_knn — and every BASELINE config) or in no order (0: a ball query)?  The weights need the largest squared distance of a case before
 * the first term can be summed (infra.pyx:668-702); sorted rows give it away (the last neighbour), unsorted rows cost a pass of their own.
 * The staged kernels of the small dense systems have a form for either (csrc/fit_stage.hip) and the CALLER's word picks it — the time of a
 * call is a function of its arguments, not of what ran before it on the stream.  A hint, never a condition of correctness: the kernels verify
 * the order bit for bit and the results are the same bits either way.  Belongs to the calling thread; returns the previous value. */
int wlsqm_hip_set_order_hint(int sorted);

/* Test hook of the strict mode: runs the reference-order fit of `b` (uniform order) and also stores the reference's intermediates,
 * for bit-for-bit comparison with values captured from the reference (tests/golden/sweep_*.npz): w[j * w_stride + k]
 * (Case_make_weights), the unscaled A and the scaled LU factor as nr x nr Fortran-order blocks at [j * mat_stride]
 * (make_A impl.pyx:566-602; dgetrf), row_scale / col_scale (Ruiz) and the 1-based ipiv at [j * vec_stride + i]. */
int wlsqm_hip_strict_intermediates_device(const wlsqm_batch* b, int device, void* stream, int order_uniform,
                                          double* w, int64_t w_stride, double* A, double* LU, int64_t mat_stride,
                                          double* row_scale, double* col_scale, int32_t* ipiv, int64_t vec_stride);

/* Index-based ("cloud") variant of wlsqm_hip_fit_many_device — an EXTENSION of the reference surface (the step
 * before the path: examples/expertsolver_example.py:91-92 builds xk = S[hoods], fk = F[hoods] on the host).
 * The kernels gather the neighbour rows themselves from the device-resident point tables S[npoints, dim] and
 * F[npoints] through hoods[ncases, max_nk] (int32), which cuts the algorithmic HBM bytes per fit from
 * 8 nk (dim+1) to 4 nk.  xi of case j is S[point_index ? point_index[j] : j].  All cases have polynomial order
 * `order`; nk / knowns / weighting_method are per-case device arrays (unit stride); fi is in/out as usual.
 * Only the slots k < nk[j] of a hoods row are dereferenced: the padding of a ragged row may hold anything (-1, npoints,
 * ...), as with the reference's dense arrays (simple.pyx:147).  Slots k < nk[j] must be valid point numbers.
 * iterations_out as for wlsqm_hip_fit_many_device (NULL: nothing but kernel launches).
 * Every (dimension, order); with sensitivities or refinement only systems with no <= 15 DOFs (not 3D order 3/4). */
int wlsqm_hip_fit_cloud_device(int dimension, int order, int64_t ncases, int64_t max_nk,
                               const double* S, const double* F, const int32_t* hoods, int64_t hoods_stride_case,
                               const int32_t* point_index, const int32_t* nk, const int64_t* knowns,
                               const int32_t* weighting_method, double* fi, int64_t fi_stride_case,
                               double* sens, int64_t sens_stride_case, int64_t sens_stride_k, int do_sens,
                               int iterative, int max_iter, int device, void* stream, int32_t* iterations_out);

/* ---- the adjoint of the fit (extension; csrc/fit_adjoint.hip) ----
 * The fit is a linear map of its data (fk and the known entries of fi); these two functions apply its transpose.  Given
 * g[j * g_stride_case + a] = dL/dfi_out[j, a] for the number_of_dofs(dimension, order) DOFs of every case, they write
 *   grad_fk[j * gfk_stride_case + k * gfk_stride_k] = dL/dfk[j, k] for EVERY k < max_nk: exact zeros for nk[j] <= k (the caller's
 *     buffer may hold anything), and a whole row of zeros for a case with every DOF known (the fit's no-op);
 *   grad_fi[j * gfi_stride_case + a] = dL/dfi_in[j, a]: g[j, a] minus the fit's dependence on that value for a true known, g[j, a] for a
 *     DOF dropped by stray high mask bits (it leaves the fit as it came in), 0 for an unknown (its incoming value is never read).
 *     grad_fi may be NULL (not wanted), and may alias g: each case reads its row of g before it writes.
 * Of `b` the geometry is read — dimension, ncases, xk, nk, xi, knowns, weighting_method, max_nk with their strides; b->fk, b->fi,
 * b->sens and b->order are NOT read (the Jacobian depends on the geometry, the weights and the mask only) and may be NULL;
 * b->iterative and b->do_sens must be 0 (WLSQM_EVALUE: the refinement's stop test is data-dependent, it has no adjoint here).
 * order_uniform, case_index / nsel, device and stream as for wlsqm_hip_fit_many_device.  Nothing but one kernel launch: no
 * allocation, no host synchronisation, no state; it can be captured into a hipGraph.  The arithmetic is always the fast kernels'
 * (FMA, LDL^T), whatever the calling thread's numerics mode: the four modes round the same linear map differently.
 * 1D orders 0-4, 2D orders 0-4, 3D orders 0-2; 3D orders 3 and 4: WLSQM_EVALUE, "fit_adjoint: unsupported (dimension, order)". */
int wlsqm_hip_fit_adjoint_device(const wlsqm_batch* b, int device, void* stream, int order_uniform,
                                 const double* g, int64_t g_stride_case,
                                 double* grad_fk, int64_t gfk_stride_case, int64_t gfk_stride_k,
                                 double* grad_fi, int64_t gfi_stride_case,
                                 const int64_t* case_index, int64_t nsel);

/* The same for index-based input: the geometry arguments of wlsqm_hip_fit_cloud_device (F, fi, sens and the refinement are not
 * part of it).  grad_slots[j * gs_stride_case + k] = dL/dF[hoods[j, k]] contributed by case j, for every k < max_nk (zeros from
 * nk[j] on; the padding of a hoods row is never dereferenced); summing the slots into dL/dF (npoints) is the caller's scatter.
 * g, grad_fi (nullable, may alias g) as above. */
int wlsqm_hip_fit_cloud_adjoint_device(int dimension, int order, int64_t ncases, int64_t max_nk,
                                       const double* S, const int32_t* hoods, int64_t hoods_stride_case,
                                       const int32_t* point_index, const int32_t* nk, const int64_t* knowns,
                                       const int32_t* weighting_method,
                                       const double* g, int64_t g_stride_case, double* grad_slots, int64_t gs_stride_case,
                                       double* grad_fi, int64_t gfi_stride_case, int device, void* stream);

/* ---- the geometry adjoint of the fit (extension; csrc/fit_adjoint.hip) ----
 * The gradient of L = g . fi_out with respect to the COORDINATES of a basic fit, which the fit is not linear in.  Per case, with
 * d_k = xk_k - xi, c_k the scaled monomials of d_k, U / Kn / D the unknown, truly known and dropped DOFs, phi = fi_out with the entries
 * in D replaced by 0, y_U = M_UU^-1 g_U (y = 0 outside U), s_k = c_k . y, r_k = fk_k - c_k . phi, and (d_m c)[a] the scaled monomial
 * whose exponent on axis m is one lower (0 when that exponent is 0), for k < nk[j]:
 *   e[k][m] = (dw_k/dd_k,m) s_k r_k + w_k ( r_k (d_m c_k . y) - s_k (d_m c_k . phi) ).
 * Uniform weights: dw = 0.  Otherwise (alpha = 1e-4, beta = 1 - alpha), D2 = max_k d2_k, rho_k = sqrt(d2_k / D2), t_k = 1 - rho_k:
 *   dw_k/dd_k,m = -2 beta t_k d_k,m / (rho_k D2),
 *   E           = sum_k (beta t_k rho_k / D2) s_k r_k,
 *   e[k*][m]   += 2 d_k*,m E          (D2 moves with the farthest neighbour k* only).
 * Outputs: grad_xk[j, k, m] = e[k][m] for k < nk[j] and EXACT ZEROS for nk[j] <= k < max_nk; grad_xi[j, m] = -sum_k e[k][m];
 * grad_fk[j, k] = w_k s_k (nullable: not wanted; for the systems up to 10 unknowns the bits of wlsqm_hip_fit_adjoint_device's).
 * A case with every DOF known has zeros everywhere.  The fit is not smooth at two kinds of point, and the conventions there are:
 *   - a neighbour ON xi (rho_k == 0): the cone of |d| at d = 0 contributes 0 (dw_k/dd_k = 0);
 *   - a tie for the farthest neighbour: k* is the SMALLEST index that attains D2 in the kernel's own fp64 squared distances.
 * Of `b`: the geometry as for wlsqm_hip_fit_adjoint_device, and b->fk (read) and b->fi, the output of the forward call (read, never
 * written); b->sens and b->order are not read; b->iterative and b->do_sens must be 0 (WLSQM_EVALUE).  grad_xk has a case and a slot
 * stride (the `dimension` coordinates of a slot contiguous), grad_xi a case stride, grad_fk a case and a slot stride; none may alias an
 * input.  g, order_uniform, case_index / nsel, device and stream as for wlsqm_hip_fit_adjoint_device.  Nothing but one kernel launch
 * (wlsqm_hip_last_kernel(): "geometry-adjoint-lane" or "geometry-adjoint-rows"): no allocation, no host synchronisation, no state; it
 * can be captured into a hipGraph.  The arithmetic is always the fast kernels'.  1D orders 0-4, 2D orders 0-4, 3D orders 0-2; 3D orders
 * 3 and 4: WLSQM_EVALUE, "fit_geometry_adjoint: unsupported (dimension, order)". */
int wlsqm_hip_fit_geometry_adjoint_device(const wlsqm_batch* b, int device, void* stream, int order_uniform,
                                          const double* g, int64_t g_stride_case,
                                          double* grad_xk, int64_t gxk_stride_case, int64_t gxk_stride_k,
                                          double* grad_xi, int64_t gxi_stride_case,
                                          double* grad_fk, int64_t gfk_stride_case, int64_t gfk_stride_k,
                                          const int64_t* case_index, int64_t nsel);

/* The same for index-based input: the arguments of wlsqm_hip_fit_cloud_device (F is read; fi is the forward call's output, read and
 * never written).  grad_slots[j * gs_stride_case + k * dimension + m] = dL/dS[hoods[j, k], m] contributed by slot k of case j, for every
 * k < max_nk (zeros from nk[j] on; the padding of a hoods row is never dereferenced); grad_own[j * go_stride_case + m] = dL/dS of the
 * case's own point (point_index[j], or j), m < dimension; grad_F_slots[j * gfs_stride_case + k] (nullable) = dL/dF[hoods[j, k]] as
 * wlsqm_hip_fit_cloud_adjoint_device writes it.  Summing slots and own rows into dL/dS (npoints, dimension) is the caller's scatter. */
int wlsqm_hip_fit_cloud_geometry_adjoint_device(int dimension, int order, int64_t ncases, int64_t max_nk,
                                                const double* S, const double* F, const int32_t* hoods, int64_t hoods_stride_case,
                                                const int32_t* point_index, const int32_t* nk, const int64_t* knowns,
                                                const int32_t* weighting_method, const double* fi, int64_t fi_stride_case,
                                                const double* g, int64_t g_stride_case,
                                                double* grad_slots, int64_t gs_stride_case, double* grad_own, int64_t go_stride_case,
                                                double* grad_F_slots, int64_t gfs_stride_case, int device, void* stream);

/* ---- ExpertSolver (expert.pyx:66-781): handle-based prepare-once / solve-many ---- */
typedef struct wlsqm_expert wlsqm_expert;

/* expert.pyx:92-264 __init__: host arrays nk/order/knowns/weighting_method of length ncases. */
int wlsqm_hip_expert_create(wlsqm_expert** out, int device, int dimension, int64_t ncases,
                            const int32_t* nk, const int32_t* order, const int64_t* knowns,
                            const int32_t* weighting_method, int algorithm, int do_sens, int max_iter);
/* expert.pyx:92-93, 112-126, 163-189, 243-252 ExpertSolver(..., host=other): "guest mode".  The new solver shares the
 * host's device-resident geometry and per-case metadata (nk, order, knowns, weighting_method) instead of holding a copy,
 * and owns only its field buffers (fk, fi, sens).  The host must be prepared (WLSQM_ERUNTIME otherwise, as the
 * reference's RuntimeError).  The shared state is reference-counted: destroying the host first is safe. */
int wlsqm_hip_expert_create_guest(wlsqm_expert** out, wlsqm_expert* host, int algorithm, int do_sens, int max_iter);
/* expert.pyx:309-426 prepare(xi, xk): host arrays; geometry is uploaded and kept device-resident.  On a guest the
 * arrays are ignored (expert.pyx:350-352: the host's geometry is used) and only the host's ready state is checked. */
int wlsqm_hip_expert_prepare(wlsqm_expert* h, const double* xi, int64_t xi_stride_case,
                             const double* xk, int64_t xk_stride_case, int64_t xk_stride_k, int64_t max_nk);
/* Extension: prepare() from device-resident arrays (xi[ncases, xi_stride_case], xk[ncases, xk_stride_case / dimension,
 * dimension] with xk_stride_k == dimension); the geometry is copied device-to-device on `stream` into the solver's own block.
 * The calling thread's wlsqm_hip_set_order_hint is recorded with the geometry (the host form looks at the rows itself). */
int wlsqm_hip_expert_prepare_device(wlsqm_expert* h, void* stream, const double* xi, int64_t xi_stride_case,
                                    const double* xk, int64_t xk_stride_case, int64_t xk_stride_k);
/* expert.pyx:467-655 solve(fk, fi, sens): host arrays; returns max iterations via *iterations_out. */
int wlsqm_hip_expert_solve(wlsqm_expert* h, const double* fk, int64_t fk_stride_case, int64_t fk_stride_k,
                           double* fi, int64_t fi_stride_case,
                           double* sens, int64_t sens_stride_case, int64_t sens_stride_k,
                           int32_t* iterations_out);
/* Device-resident variant of solve(): fk [ncases,max_nk] and fi [ncases,fi_stride_case] are device
 * pointers (contiguous k axis); enqueued on `stream`; no host synchronisation.  fi must be at least max_no doubles wide
 * (every row is written at fi_stride_case pitch).  As in the reference, interpolate() afterwards evaluates the coefficients
 * of the LATEST solve of any kind: after this call that is the caller's `fi` array itself (no copy is made), so it must
 * stay allocated until the next solve or until interpolation is no longer used. */
int wlsqm_hip_expert_solve_device(wlsqm_expert* h, void* stream, const double* fk, int64_t fk_stride_case,
                                  double* fi, int64_t fi_stride_case);
/* Extension: the neighbour search the reference's examples run on the host before calling the fitter
 * (examples/expertsolver_example.py:48-66: cKDTree(x).query(x, 1 + nk), the point itself dropped;
 * examples/wlsqm_example.py:103-133).  For every point of the device-resident cloud S[npoints, dimension] the k nearest
 * OTHER points, ascending by (distance, index), into the device array hoods[npoints, k] (int32) — the `hoods` argument of
 * wlsqm_hip_fit_cloud_device.  Exact (uniform-grid search with a provable stop test).  1 <= k <= min(npoints - 1, 213).
 * Synchronises `stream` before returning.
 * Domain of this and the three searches below: finite coordinates (a NaN or an infinity anywhere in S is WLSQM_EVALUE,
 * "non-finite coordinates") whose bounding box has a representable squared diagonal (else WLSQM_EVALUE: every squared distance
 * would be inf).  Squared distances must not underflow either: points closer than about 2^-511 on every axis count as
 * coincident.  Coincident points are legal; they tie, and ties are ordered by index. */
int wlsqm_hip_knn_device(int dimension, int64_t npoints, const double* S, int k, int32_t* hoods, int device, void* stream);
/* Extension: the same search asked only by the FIRST nquery points of the cloud; the remaining npoints - nquery points are
 * candidates only (hoods[nquery, k], indices into S).  The rank of a partitioned cloud searches its own points against its
 * own points plus a halo band of its neighbours' (wlsqm/sharded.py) instead of the global cloud. */
int wlsqm_hip_knn_subset_device(int dimension, int64_t npoints, const double* S, int k, int64_t nquery, int32_t* hoods,
                                int device, void* stream);
/* Extension: the radius form of the same search (examples/wlsqm_example.py:103-133: query_ball_point(x, r), at most
 * max_nk neighbours kept).  For every point the other points within `radius`, nearest first, at most max_nk of them:
 * hoods[npoints, max_nk] (int32; unused slots hold the point's own index) and nk[npoints] (int32, the counts). */
int wlsqm_hip_ball_device(int dimension, int64_t npoints, const double* S, double radius, int max_nk,
                          int32_t* hoods, int32_t* nk, int device, void* stream);
/* Extension: nearest point of the device-resident cloud S[ndata, dimension] for each of the device-resident query points
 * X[nquery, x_stride] (queries are not members of the cloud): nearest[nquery] (int64 device array, indices into S; ties go
 * to the smaller index).  What ExpertSolver.interpolate(mode='nearest') needs (cKDTree.query in expert.pyx:830-895).
 * A query with a NaN coordinate, or one so far away that its squared distances overflow, has no nearest point: it gets
 * 2^31 - 1, which is no index of S (an interpolation plan evaluates to NaN there). */
int wlsqm_hip_nearest_device(int dimension, int64_t ndata, const double* S, int64_t nquery, const double* X,
                             int64_t x_stride, int64_t* nearest, int device, void* stream);
/* Extension: the shape of the uniform grid that the four searches above lay over a cloud of npoints points with the bounding
 * box lo[dimension] .. hi[dimension]: g[dimension] cells per axis of side cell[dimension], about 4 points per cell, at most
 * 2^27 cells in all.  Host arithmetic only: needs no device.  WLSQM_EVALUE for a box outside the searches' domain. */
int wlsqm_hip_grid_shape_host(int dimension, int64_t npoints, const double* lo, const double* hi, int32_t* g, double* cell);

/* Extension: the Morton order of the device-resident cloud S[npoints, dimension] (csrc/order.hip states the order; DESIGN.md
 * section 23).  perm[npoints] (int32, device): new position i holds old point perm[i], the stable ascending sort of the keys
 * (ties go to the smaller old index); inverse[npoints] (int32, device): inverse[perm[i]] = i; keys_sorted[npoints] (int64,
 * device, nullable): the keys in ascending order; box[2][3] (HOST doubles): the bounding box, lo then hi, that the keys were
 * taken under.  2D / 3D: 31 / 21 bits per axis of floor((x - lo) / (hi - lo) * 2^B), interleaved (axis 0 lowest); 1D: the
 * exact order of the doubles.  1 <= npoints < 2^31; S in the domain of wlsqm_hip_knn_device (the same WLSQM_EVALUE and words
 * otherwise).  Allocates and frees its temporaries; synchronises `stream` before returning. */
int wlsqm_hip_spatial_order_device(int dimension, int64_t npoints, const double* S, int64_t* keys_sorted, int32_t* perm,
                                   int32_t* inverse, double* box, int device, void* stream);
/* Extension: the keys of ANY device-resident points X[n, dimension] under the box lo[dimension] .. hi[dimension] (host arrays;
 * the box of wlsqm_hip_spatial_order_device places new points in an existing order): keys[n] (int64, device).  Points outside
 * the box clamp to its ends; a NaN coordinate gives the largest key of the dimension (2^62 - 1, 2^63 - 1; 1D: 2^63 - 1).
 * Asynchronous, allocates nothing, legal during stream capture. */
int wlsqm_hip_spatial_keys_device(int dimension, int64_t n, const double* X, const double* lo, const double* hi, int64_t* keys,
                                  int device, void* stream);
/* Extension: renumber neighbour lists.  out[i, k] = inverse[hoods[r, k]] for k < nk[r], where r = row_perm[i] (row_perm
 * nullable: r = i; a permutation of 0 .. ncases - 1 otherwise) and nk is nullable (every slot is live).  hoods[ncases, K] at a
 * pitch of row_stride >= K, out[ncases, K] at a pitch of K, inverse[npoints], all int32 on the device.  The padding slots
 * k >= nk[r] get own[i] (own nullable: i), the way wlsqm_hip_ball_device pads its rows.  A live entry outside
 * 0 .. npoints - 1 is never dereferenced: it is written as -1 and counted in *bad (a device int32 that the CALLER has set,
 * nullable), and so is every slot of a row whose row_perm entry is no row.  Asynchronous, allocates nothing, legal during
 * stream capture. */
int wlsqm_hip_relabel_hoods_device(int64_t ncases, int K, const int32_t* hoods, int64_t row_stride, const int32_t* nk,
                                   const int32_t* row_perm, const int32_t* inverse, int64_t npoints, const int32_t* own,
                                   int32_t* out, int32_t* bad, int device, void* stream);

/* Extension: build the stored solution operator of the prepared geometry now (8 x 16 x K' bytes per case, K' = the neighbour
 * slots rounded up to a multiple of 8; shared with guests), so that later stacked solves only enqueue work — e.g. before a stream
 * capture.  Without this call the first wlsqm_hip_expert_solve_many[_device] that wants the operator builds it and synchronises
 * `stream`.  *built = 1 when the operator exists afterwards, 0 when the shape has none (more than 15 unknowns, more than 64 or an
 * odd number of slots, more than 4 knowns per case, mixed orders, ALGO_ITERATIVE) or it does not fit the free device memory: the
 * stacked solve then takes its other kernels. */
int wlsqm_hip_expert_prepare_operator(wlsqm_expert* h, void* stream, int* built);
/* Extension (no reference counterpart; BASELINE config 4 "prepare once + 256 RHS solves"): nrhs fields on the prepared
 * geometry in one call.  Equivalent to nrhs calls of expert.pyx:467-655 solve() with ALGO_BASIC and no sensitivities,
 * in one launch: stacks of 64 fields or more, and every stack on a shape with more than 6 unknowns or 32 neighbour slots,
 * apply the stored solution operator (wlsqm_hip_expert_prepare_operator; csrc/solve_op.hip, one batched GEMM on the matrix
 * cores); short stacks on small shapes share the geometry work (weights, monomials, normal matrix, factorisation) inside the
 * launch (csrc/solve_many.hip); anything else runs one fused launch per field.  Device variant: fk[nrhs][ncases][max_nk]
 * and fi[nrhs][ncases][fi_stride_case] are device pointers with the given element strides (k contiguous), enqueued on
 * `stream`.  Host variant: strided host arrays, transferred in chunks of right-hand sides. */
int wlsqm_hip_expert_solve_many_device(wlsqm_expert* h, void* stream, int64_t nrhs,
                                       const double* fk, int64_t fk_stride_rhs, int64_t fk_stride_case,
                                       double* fi, int64_t fi_stride_rhs, int64_t fi_stride_case);
int wlsqm_hip_expert_solve_many(wlsqm_expert* h, int64_t nrhs,
                                const double* fk, int64_t fk_stride_rhs, int64_t fk_stride_case, int64_t fk_stride_k,
                                double* fi, int64_t fi_stride_rhs, int64_t fi_stride_case);
/* Extension: the adjoint (vector-Jacobian product) of wlsqm_hip_expert_solve_many_device on the prepared geometry (csrc/solve_op.hip,
 * csrc/fit_adjoint.hip).  g[nrhs][ncases][g_stride_case] = dL/dfi_out (device, DOF axis contiguous).  Writes
 * grad_fk[r][j][k] = dL/dfk for EVERY k < gfk_slots (gfk_slots >= max(nk); exact zeros from nk[j] on and for a case with every DOF
 * known) and, when grad_fi is not NULL, grad_fi[r][j][a] = dL/dfi_in for every a < no[j] (0 for an unknown, g for a DOF dropped by
 * stray high mask bits, g minus the fit's dependence on the value for a known DOF; columns beyond no[j] are untouched).  g, grad_fk
 * and grad_fi must not overlap.  Two routes to the same numbers: the stored operator's transpose as one batched GEMM on the matrix
 * cores (wlsqm_hip_last_kernel(): "solve-op-adjoint-mfma"; the shapes of wlsqm_hip_expert_prepare_operator, grad_fk 16-byte aligned
 * with even strides and an even gfk_slots), or one adjoint of the fit per field on the resident geometry (every other case; mixed
 * orders in buckets).  The operator is built on demand as for the stacked solve (that call synchronises `stream`) but never while
 * `stream` is capturing; with the operator present the call only enqueues kernels.  Always the fast arithmetic, whatever the
 * numerics mode.  WLSQM_ERUNTIME before prepare(); WLSQM_EVALUE for an ALGO_ITERATIVE solver (the stop test is data-dependent) and
 * for 3D orders 3 and 4 ("fit_adjoint: unsupported (dimension, order)"). */
int wlsqm_hip_expert_solve_adjoint_device(wlsqm_expert* h, void* stream, int64_t nrhs,
                                          const double* g, int64_t g_stride_rhs, int64_t g_stride_case,
                                          double* grad_fk, int64_t gfk_stride_rhs, int64_t gfk_stride_case, int64_t gfk_slots,
                                          double* grad_fi /* nullable */, int64_t gfi_stride_rhs, int64_t gfi_stride_case);
/* expert.pyx:429-464 conds(): 2-norm condition number of the Ruiz-scaled reduced matrix of every case
 * (impl.pyx:662-682), out[ncases] on the host.  Diagnostics path (one-sided Jacobi SVD per case). */
int wlsqm_hip_expert_conds(wlsqm_expert* h, double* out);
/* expert.pyx:687-781 interpolate(): evaluate the models of the last solve() (or their derivative `diff`, a DOF
 * index) at nx host points x[nx, dim].  mode='nearest': I[nx] (host) names the model per point (expert.pyx:830-895;
 * the nearest-origin search itself stays on the host, scipy cKDTree, as in the reference); mode='continuous':
 * CSR lists list_off[nx+1], list_idx[] of the models within radius r of each point (expert.pyx:898-985). */
int wlsqm_hip_expert_interpolate(wlsqm_expert* h, const double* x, int64_t x_stride, int64_t nx, const int64_t* I,
                                 const int64_t* list_off, const int64_t* list_idx, double r, int diff, double* out);
/* mode='nearest' with the nearest-origin search on the device too (the reference queries a cKDTree of the origins,
 * expert.pyx:830-895): out[nx] the values, I_out[nx] (nullable) the model chosen for every point. */
int wlsqm_hip_expert_interpolate_nearest(wlsqm_expert* h, const double* x, int64_t x_stride, int64_t nx, int diff,
                                         double* out, int64_t* I_out);
/* mode='continuous' with the ball search on the device too (the reference builds the lists with
 * cKDTree.query_ball_tree, expert.pyx:898-903): out[nx] = weighted average (weights (1 - d/r)^2, expert.pyx:45-46)
 * of the models whose origin lies within r of the point; NaN where there is none. */
int wlsqm_hip_expert_interpolate_continuous(wlsqm_expert* h, const double* x, int64_t x_stride, int64_t nx, double r,
                                            int diff, double* out);
/* expert.pyx:289-306 memory_used(): (bytes in use, bytes reserved) of the device-side state; a guest counts only
 * what it owns (the shared geometry is the host's). */
int wlsqm_hip_expert_memory_used(const wlsqm_expert* h, int64_t* used, int64_t* total);
/* expert.pyx:267-286 __del__ */
int wlsqm_hip_expert_destroy(wlsqm_expert* h);

/* ---- model evaluation (the step after the path) ---- */
/* interp.pyx:34-143 interpolate_fit: one model (xi[dim], fi[no], order) or its derivative `diff` at nx host points. */
int wlsqm_hip_interpolate_fit_host(int dimension, int order, const double* xi, const double* fi,
                                   const double* x, int64_t x_stride, int64_t nx, int diff, double* out, int device);

/* ---- interpolation plans (extension): search once, evaluate many times, device-resident (csrc/interp_plan.hip) ----
 * A plan holds everything about "these models evaluated at these points" that does not depend on the coefficients: its own
 * packed copies of the origins xi[nmodels, dimension], the orders and the points x[nx, dimension], and per point the model
 * number (mode 0 = nearest: the nearest origin, ties to the smaller index, or the caller's I_dev) or the list of the models
 * whose origin lies within r (mode 1 = continuous).  The caller's arrays may be freed after create.
 *
 * create: all pointers are DEVICE pointers; strides in elements, rows of `dimension` contiguous coordinates.  order_dev: one
 * int32 per model, or order_stride 0 for one shared value.  I_dev (nullable, nearest only): the model per point given by the
 * caller instead of searched.  r is read in continuous mode only.  May allocate and synchronises `stream`, as prepare() does.
 * WLSQM_EVALUE on a bad dimension, mode or order, r <= 0 (continuous), nmodels outside 1 .. 2^31 - 1, nx outside 0 .. 2^31 - 2,
 * non-finite origins where they are searched, or I_dev in continuous mode; WLSQM_EMEMORY when the lists do not fit.
 * create_expert: the origins and orders of the solver's prepared geometry (WLSQM_ERUNTIME before prepare()); the plan keeps
 * copies and does not refer to the solver afterwards.
 *
 * Lists (continuous): int32 model numbers in CSR form.  Within a point the models come in the order of the grid walk: the
 * cells of the uniform grid over the origins in ascending (z, y, x), the origins of one cell in ascending model number — a
 * function of the inputs alone, so two plans of the same inputs hold identical lists.
 *
 * eval_*: out[f][d][m] = d^diffs[d] model(x_m) of field f, at out + f * out_stride_field + d * out_stride_diff + m; the
 * coefficients of model j of field f are fi + f * fi_stride_field + j * fi_stride_model, at least `no` of them.  diffs is a
 * HOST array of DOF numbers, ndiff <= 35, passed to the kernel by value.  Semantics as wlsqm_hip_expert_interpolate: a diff
 * that is negative or >= the model's number of DOFs gives 0, a model number outside 0 .. nmodels - 1 gives NaN, the
 * continuous weight is (1 - sqrt(d2 / r2))^2 and an empty list gives NaN.  A value does not depend on what else the call
 * asks for: the result for (point, field, diff) is bit-identical whether the diff is asked alone or among others, in any
 * position or repeated, whether the field is alone or in a stack, eager or replayed from a graph.
 * The eval calls ONLY ENQUEUE one kernel on `stream`: no allocation, no host synchronisation, no copy — they are legal inside
 * a stream capture.  Ordering against the work that produces fi (a solve_device on another stream, say) is plain stream
 * order and is the CALLER's business: enqueue the evaluation on the stream of the solve, or make that stream wait for it.
 * nx == 0 or ndiff == 0 is a no-op that returns WLSQM_OK.
 * eval_expert evaluates the coefficients of the solver's latest solve of any kind (after solve_device that is the caller's
 * own array, which must still be allocated); WLSQM_ERUNTIME before the first solve. */
typedef struct wlsqm_interp_plan wlsqm_interp_plan;
int wlsqm_hip_interp_plan_create(wlsqm_interp_plan** out, int device, void* stream, int dimension, int64_t nmodels,
                                 const double* xi_dev, int64_t xi_stride, const int32_t* order_dev, int64_t order_stride,
                                 int mode, const double* x_dev, int64_t x_stride, int64_t nx, double r, const int64_t* I_dev);
int wlsqm_hip_interp_plan_create_expert(wlsqm_interp_plan** out, wlsqm_expert* h, void* stream, int mode,
                                        const double* x_dev, int64_t x_stride, int64_t nx, double r, const int64_t* I_dev);
/* every output is nullable: points, list entries in all, the longest list, device bytes the plan holds */
int wlsqm_hip_interp_plan_info(const wlsqm_interp_plan* plan, int64_t* nx, int64_t* nlist, int64_t* max_list, int64_t* bytes);
/* nearest: I_dev[nx]; continuous: off_dev[nx + 1], idx_dev[nlist] (int64 device arrays, for inspection and for feeding
 * wlsqm_hip_expert_interpolate's lists); enqueued on `stream` */
int wlsqm_hip_interp_plan_export(const wlsqm_interp_plan* plan, void* stream, int64_t* I_or_off_dev, int64_t* idx_dev);
int wlsqm_hip_interp_plan_eval_device(const wlsqm_interp_plan* plan, void* stream, int64_t nfields,
                                      const double* fi_dev, int64_t fi_stride_field, int64_t fi_stride_model,
                                      const int32_t* diffs, int ndiff, double* out_dev, int64_t out_stride_field,
                                      int64_t out_stride_diff);
int wlsqm_hip_interp_plan_eval_expert(const wlsqm_interp_plan* plan, wlsqm_expert* h, void* stream, const int32_t* diffs,
                                      int ndiff, double* out_dev, int64_t out_stride_diff);
int wlsqm_hip_interp_plan_destroy(wlsqm_interp_plan* plan);

/* ---- the adjoint of the evaluation (extension) ----
 * eval_* is linear in fi, so its adjoint takes g[f][d][m] = dL/d out[f][d][m] (at g_dev + f * g_stride_field + d * g_stride_diff + m)
 * to grad_fi[f][i][a] = dL/d fi[f][i][a] (at grad_fi_dev + f * gfi_stride_field + i * gfi_stride_model + a):
 *     nearest:     grad_fi[f][i][a] = sum over m with I_m == i, over d with P_a >= P_diffs[d]:  g[f][d][m] c_m[index(P_a - P_diffs[d])]
 *     continuous:  the same over the list entries (m, e) with idx[e] == i, every term times w_{m,e} / W_m, W_m = sum_e w_{m,e}
 * with c_m the scaled monomials of x_m - xi[i] and P the exponent table.  EVERY element of grad_fi[f][0 .. nmodels)[0 .. ncols) is
 * written (exact zeros in the columns from the model's own number of DOFs on and in the rows of models that no point uses) and
 * nothing else is; the caller pre-fills nothing.  ncols >= the number of DOFs of the plan's largest order, gfi_stride_model >= ncols.
 * A point whose value does not depend on fi (model number outside 0 .. nmodels - 1, empty list, W_m == 0) and a diff that no model of
 * the plan has contribute nothing and their g is never read; a diff given twice contributes twice.  With nx == 0 or ndiff == 0 the
 * call still writes the zeros.  ndiff in 0 .. 35, nfields >= 0 (0: nothing happens).
 * No atomics: the sum is a gather over the plan's inverted index (per model the points that use it, in ascending point number), one
 * lane per model, one wavefront per model with more than `threshold` entries (wlsqm_hip_last_kernel(): "interp-plan-adjoint",
 * "interp-plan-adjoint+wave" when the plan has such models).  The bits of grad_fi[f] are a function of the plan and of field f's g:
 * the same run to run, eager or replayed from a graph, with the field alone or anywhere in a stack, with the diffs in any order (and
 * g's diff axis permuted alike).
 * prepare_adjoint builds the inverted index now (a stable sort; it allocates and synchronises `stream`; idempotent); *built
 * (nullable) = 1 when the index exists afterwards.  Without it the first eval_adjoint_device builds the index on demand — unless
 * `stream` is capturing: then it returns WLSQM_ERUNTIME (call prepare_adjoint before the capture) with nothing enqueued.  With the
 * index present eval_adjoint_device only enqueues kernels.  WLSQM_EVALUE when the index would hold more than 2^31 - 1 entries.
 * adjoint_info (every output nullable): entries of the index, the longest list of a model, the number of models that take the wave
 * form (all three -1 while the index is absent) and the threshold.  export_transposed: toff_dev[nmodels + 1] and tpt_dev[nentries]
 * (int64 device arrays; the points of model i are tpt[toff[i] .. toff[i + 1])), enqueued on `stream`; WLSQM_ERUNTIME without index. */
int wlsqm_hip_interp_plan_prepare_adjoint(wlsqm_interp_plan* plan, void* stream, int* built);
int wlsqm_hip_interp_plan_adjoint_info(const wlsqm_interp_plan* plan, int64_t* nentries, int64_t* max_len, int64_t* nlong,
                                       int32_t* threshold);
int wlsqm_hip_interp_plan_export_transposed(const wlsqm_interp_plan* plan, void* stream, int64_t* toff_dev, int64_t* tpt_dev);
int wlsqm_hip_interp_plan_eval_adjoint_device(wlsqm_interp_plan* plan, void* stream, int64_t nfields,
                                              const int32_t* diffs, int ndiff, const double* g_dev, int64_t g_stride_field,
                                              int64_t g_stride_diff, double* grad_fi_dev, int64_t gfi_stride_field,
                                              int64_t gfi_stride_model, int ncols);

/* ---- batched dense solves: wlsqm.utils.lapackdrivers (lapackdrivers.pyx, the m* / *factor* families) ----
 * `count` independent problems in the reference's layout, Fortran order throughout: A is (n, n, nlhs) with element
 * (i, j, k) at A[i + n*j + n*n*k]; b is (n, count), ipiv (n, nlhs) int32 with LAPACK's 1-based entries, info one
 * int32 per factored matrix (LAPACK's INFO: j > 0 if the j-th pivot is exactly zero; the factorization completes).
 *   getrf / gesv: dgetf2 semantics (partial pivoting, first largest |entry| of the column).
 *   sytrf / sysv: dsytf2 semantics with uplo = 'U' (Bunch-Kaufman, 1x1 and 2x2 pivots, dsytrf's ipiv encoding); the
 *                 strict lower triangle of A is neither read nor written.
 *   getrs / sytrs: right-hand side k is solved with the factor A[:, :, k*lhs_stride] and its pivots; lhs_stride is 1
 *                 (one factor per right-hand side) or 0 (one factor for every right-hand side, nlhs = 1).
 *   gesv / sysv:  factor + solve in one launch, one right-hand side per matrix.  A, ipiv and info are written; b gets
 *                 the solution when the matrix's INFO is 0 and is left bit-unchanged otherwise (dgesv / dsysv solve only
 *                 when INFO == 0), whether or not `info` is null.
 * n >= 1, count >= 0 (0: nothing happens), null pointers -> WLSQM_EVALUE.  `info` may be null (not written).
 * The kernel that runs is a function of n alone, so a matrix gives the same bits at any position of any batch.
 * The *_device entries enqueue on `stream` without synchronising; the *_host entries take host pointers, stream them
 * through pinned staging buffers in chunks and return when the results are in the caller's arrays. */
int wlsqm_hip_getrf_batched_device(int n, int64_t count, double* A, int32_t* ipiv, int32_t* info, int device, void* stream);
int wlsqm_hip_getrs_batched_device(int n, int64_t count, int lhs_stride, const double* A, const int32_t* ipiv, double* b,
                                   int device, void* stream);
int wlsqm_hip_gesv_batched_device(int n, int64_t count, double* A, int32_t* ipiv, int32_t* info, double* b, int device,
                                  void* stream);
int wlsqm_hip_sytrf_batched_device(int n, int64_t count, double* A, int32_t* ipiv, int32_t* info, int device, void* stream);
int wlsqm_hip_sytrs_batched_device(int n, int64_t count, int lhs_stride, const double* A, const int32_t* ipiv, double* b,
                                   int device, void* stream);
int wlsqm_hip_sysv_batched_device(int n, int64_t count, double* A, int32_t* ipiv, int32_t* info, double* b, int device,
                                  void* stream);
/* A <- (A + A^T) / 2 for every matrix (the reference's msymmetrize) */
int wlsqm_hip_symmetrize_batched_device(int n, int64_t count, double* A, int device, void* stream);
int wlsqm_hip_getrf_batched_host(int n, int64_t count, double* A, int32_t* ipiv, int32_t* info, int device);
int wlsqm_hip_getrs_batched_host(int n, int64_t count, int lhs_stride, const double* A, const int32_t* ipiv, double* b,
                                 int device);
int wlsqm_hip_gesv_batched_host(int n, int64_t count, double* A, int32_t* ipiv, int32_t* info, double* b, int device);
int wlsqm_hip_sytrf_batched_host(int n, int64_t count, double* A, int32_t* ipiv, int32_t* info, int device);
int wlsqm_hip_sytrs_batched_host(int n, int64_t count, int lhs_stride, const double* A, const int32_t* ipiv, double* b,
                                 int device);
int wlsqm_hip_sysv_batched_host(int n, int64_t count, double* A, int32_t* ipiv, int32_t* info, double* b, int device);
int wlsqm_hip_symmetrize_batched_host(int n, int64_t count, double* A, int device);

/* ---- stencil operators (extension; csrc/stencil.hip) ----
 * A sparse matrix A of nrows x ncols in sliced ELLPACK with one slice per wavefront ("SELL-64"): an entry is a (column, value) pair,
 * rows are grouped in slices of 64 consecutive rows, nslices = ceil(nrows / 64).
 *   len   (nrows,)       int32    live entries of each row
 *   width (nslices,)     int32    max(len) over the slice's rows; 0 is allowed
 *   soff  (nslices + 1,) int64    entry offset of each slice; soff[s + 1] - soff[s] = 64 * width[s]
 *   col   (total,)       int32    columns, total = soff[nslices]
 *   val   (nop, total)   float64  one value plane per operator at val_stride_op (>= total); all planes share col
 * Entry e of row i sits at soff[i / 64] + 64 * e + i % 64, so a wave reads 256 contiguous bytes of col and 512 of each val plane per
 * step.  An entry with e >= len[i] is padding: neither its column nor its value is used, and X is never dereferenced for it, whatever
 * the arrays hold there (NaN and inf included).  The caller guarantees len[i] <= width[i / 64] (a longer row is cut at the width) and
 * 0 <= col < ncols for every live entry.  The writers of the layout keep the same rule from their side: wlsqm_hip_stencil_build_device
 * and wlsqm_hip_sell_permute_device (below) write live entries only and leave the padding of col and val as it is.
 *
 * wlsqm_hip_sell_apply_device:  Y[r, o, i] = alpha * sum_{e < len[i]} val[o][.] * X[r, col[.]] + beta * Y[r, o, i]  for nop >= 1
 * operators and R >= 1 stacked vectors; X[r, c] is at X[r * x_stride_field + c * x_stride_point], Y[r, o, i] at
 * Y[r * y_stride_field + o * y_stride_op + i * y_stride_row] (strides in elements).  The sum runs in entry order with fused
 * multiply-adds, so its bits are a function of the structure and the inputs; beta == 0 does not read Y.  Y must not overlap X.
 * One kernel launch on `stream`: no allocation, no synchronisation, no state; nrows == 0 launches nothing.  The transposed product is
 * the same call on the transposed matrix stored in the same format.  WLSQM_EVALUE for nop < 1, R < 1, nrows > 64 * nslices or a null
 * array. */
int wlsqm_hip_sell_apply_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                const int32_t* col, const double* val, int64_t val_stride_op, int nop,
                                int64_t R, const double* X, int64_t x_stride_field, int64_t x_stride_point,
                                double* Y, int64_t y_stride_field, int64_t y_stride_op, int64_t y_stride_row,
                                double alpha, double beta, int device, void* stream);

/* wlsqm_hip_stencil_build_device (csrc/fit_adjoint.hip): the coefficients of nop operators of the fit written straight into that layout,
 * row j = case j, one wave per slice.  The geometry arguments are those of wlsqm_hip_fit_cloud_adjoint_device; rows[o * rows_stride_op +
 * j * rows_stride_case + a] is lambda_o of case j (rows_stride_case == 0: the same operators at every case).  With n = clamp(nk[j], 0,
 * max_nk) and y_o = M_UU^-1 lambda_o (ONE factorisation per case for all operators), entry k < n of row j is
 * (hoods[j, k], w_k (c_k . y_o)): the bits of wlsqm_hip_fit_cloud_adjoint_device's grad_slots for g = lambda_o for the systems up to 10
 * unknowns; where bit F is in knowns[j], entry n is (point_index[j] or j, grad_fi[j, 0] of that call).  known_coef[o * kc_stride_op +
 * j * kc_stride_case + a] (nullable) is that call's grad_fi[j, a], column 0 zeroed where it went into the matrix.  A case with every DOF
 * known has zeros on its neighbours and lambda in the known terms.  col is nullable (not written: the neighbour lists have not changed).
 * PRECONDITION: len[j] = clamp(nk[j], 0, max_nk) + (bit F of knowns[j]) and soff is the frame of those len (nslices + 1 entries).  Entry e
 * of row j is written iff e < len[j] and e < (soff[j / 64 + 1] - soff[j / 64]) / 64; padding entries of col and val are neither read nor
 * written, the padding of a hoods row is never dereferenced.  A frame that breaks the precondition costs wrong values (entries of a
 * row left unwritten, or a row cut short) and never a write outside the arrays that soff describes.  Live entries of hoods are the
 * caller's to keep within S, as for every index-based call.  ONE kernel launch on `stream` (wlsqm_hip_last_kernel(): "stencil-build"):
 * no allocation, no synchronisation, no state; ncases == 0 launches nothing.  1D orders 0-4, 2D orders 0-4, 3D orders 0-2; otherwise
 * WLSQM_EVALUE, "fit_adjoint: unsupported (dimension, order)". */
int wlsqm_hip_stencil_build_device(int dimension, int order, int64_t ncases, int64_t max_nk,
                                   const double* S, const int32_t* hoods, int64_t hoods_stride_case,
                                   const int32_t* point_index, const int32_t* nk, const int64_t* knowns,
                                   const int32_t* weighting_method,
                                   const double* rows, int64_t rows_stride_op, int64_t rows_stride_case, int nop,
                                   const int32_t* len, const int64_t* soff, int32_t* col, double* val, int64_t val_stride_op,
                                   double* known_coef, int64_t kc_stride_op, int64_t kc_stride_case, int device, void* stream);

/* wlsqm_hip_sell_permute_device: out[o * out_stride_op + dest[e]] = in[o * in_stride_op + src[e]] for e < n and o < nop, one (dest, src)
 * pair for all planes: the values of a transposed matrix from those of the forward one.  dest must not name a position twice; positions
 * that no pair names are neither read nor written.  One kernel launch ("stencil-permute"), as above; n == 0 launches nothing. */
int wlsqm_hip_sell_permute_device(int64_t n, const int32_t* dest, const int32_t* src, const double* in, int64_t in_stride_op,
                                  double* out, int64_t out_stride_op, int nop, int device, void* stream);

/* ---- implicit solves with a stencil operator (extension; csrc/krylov.hip) ----
 * BiCGSTAB on M x = b, M = diag(d) + scale * A, A one value plane of a SQUARE matrix in the SELL-64 layout above (nrows == ncols, row i
 * the equation of point i; `val` points at the plane), d_i = diag[i] or, with diag == NULL, diag_const.  jacobi != 0: right-preconditioned
 * with the inverse of M's diagonal, d_i + scale * (the sum of row i's entries in column i, in entry order), recomputed by every start.
 * All state lives in `workspace`, wlsqm_hip_krylov_workspace_bytes(nrows) bytes of device memory, 8-byte aligned, which the caller keeps
 * from start to the last read; b, x, diag and the workspace must not overlap.  Its first 128 bytes are the scalars:
 *   double rho, rho_old, alpha, omega, rr, stop, dot0, dot1;  int32 iterations, status, done, maxiter;
 * rr = (r, r) of the recursive residual, stop = max(rtol * ||b||_2, atol), the solve stops when sqrt(rr) <= stop.  status: -1 running,
 * 0 converged, 1 iteration limit, 2 breakdown (rho == 0 or (r0, v) == 0), 3 a non-finite scalar, 4 a zero or non-finite Jacobi diagonal
 * (found before the first iteration: x stays as given).  Every status >= 0 sets `done`, and every kernel returns at its head when `done`
 * is set: iterations enqueued behind a stopped solve leave x and the scalars untouched.  b == 0 with x == 0 converges at 0 iterations
 * without a division; (t, t) == 0 takes omega = 0.  The padding of col and val and rows beyond nrows are neither read nor written.
 * Every dot product is summed in a fixed order without atomics: the bits of x and of the scalars are a function of the arguments.
 * The calls do nothing but kernel launches on `stream` (wlsqm_hip_last_kernel(): "krylov-diag", "krylov-spmv-dot", "krylov-update",
 * "krylov-reduce"): no allocation, no synchronisation, no host state.  WLSQM_EVALUE for nrows < 1, nrows > 64 * nslices, a null array,
 * rtol or atol negative or not finite, maxiter or niter negative.
 *
 * wlsqm_hip_krylov_start_device: the Jacobi diagonal, r = r0 = b - M x, the scalars and the threshold (at most 4 launches).
 * wlsqm_hip_krylov_bicgstab_device: `niter` iterations behind a start with the same arguments, 8 launches each; the solve stops by
 *   itself at convergence, at the start's maxiter or at a breakdown.
 * wlsqm_hip_krylov_product_device: the solve's fused product on its own, out = M in with dot0 = (out, w) and dot1 = (out, out) left in
 *   the scalars (2 launches; it uses the workspace's partial sums, so not between a start and the end of its solve).
 * wlsqm_hip_krylov_grads_device ("krylov-grads"): the gradients of a loss L through the solve, from x and the
 *   solution lam of M^T lam = dL/dx, in one pass over the forward matrix.  Each output is optional (NULL / 0):
 *     grad_val (total doubles, one plane in the layout of `val`): -((scale * lam[j]) * x[col]) at every live entry of row j, two
 *       roundings; +0.0 in every padding position, the lanes of rows beyond nrows included;
 *     grad_diag (nrows): -(lam[j] * x[j]);
 *     want_scale: dot0 of the scalars = -(lam, A x), the row sums those of the product, summed in the fixed order of the dot products.
 *   One launch, and the reduce when want_scale is set; not between a start and the end of its solve.  lam, x and the outputs must not
 *   overlap.  WLSQM_EVALUE as above, for a null lam or x, and when no output is asked for. */
int64_t wlsqm_hip_krylov_workspace_bytes(int64_t nrows);
int wlsqm_hip_krylov_start_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                  const int32_t* col, const double* val, const double* diag, double diag_const, double scale, int jacobi,
                                  const double* b, const double* x, double rtol, double atol, int64_t maxiter, void* workspace,
                                  int device, void* stream);
int wlsqm_hip_krylov_bicgstab_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                     const int32_t* col, const double* val, const double* diag, double diag_const, double scale, int jacobi,
                                     double* x, int64_t niter, void* workspace, int device, void* stream);
int wlsqm_hip_krylov_product_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                    const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                    const double* in, const double* w, double* out, void* workspace, int device, void* stream);
int wlsqm_hip_krylov_grads_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                  const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                  const double* lam, const double* x, double* grad_val, double* grad_diag, int want_scale,
                                  void* workspace, int device, void* stream);

/* ---- block-Jacobi preconditioner of those solves (extension; csrc/krylov.hip) ----
 * P = blockdiag(M_BB)^-1 in place of the inverse diagonal: block B is rows and columns B * block .. B * block + block - 1 of M, block one of
 * 8, 16, 32 (each divides 64: a block never crosses a slice), the last block cut at nrows and completed by the identity.  Entry (i, j) of a
 * block is d_i delta_ij + scale * (the sum of row i's entries in column j, in entry order).  nslices must be ceil(nrows / 64).
 * The block plane: wlsqm_hip_krylov_block_bytes(nrows, block) bytes of device memory, 8-byte aligned,
 *   W[(slice * block + j) * 64 + lane]   float64   entry (lane % block, j) of the inverse of the block that holds row slice * 64 + lane,
 * nslices * block * 64 doubles, so that a wave reads column j of its slice as one contiguous run of 512 bytes; rows beyond nrows are
 * identity rows.  Behind them ceil(nrows / 256) doubles: the counts of unusable blocks of the last factor, one per workgroup.
 *
 * wlsqm_hip_krylov_block_factor_device ("krylov-blocks", one launch): gathers every diagonal block from the matrix and inverts it by
 *   Gauss-Jordan elimination with partial row pivoting (the largest entry of the column among the rows not yet used, the lowest row at a
 *   tie), one lane per row.  planes_t (nullable): a second plane that receives the transposed inverses, the preconditioner of M^T.  A zero
 *   or non-finite pivot or a non-finite inverse counts the block as unusable: never a fault, and the next start answers status 4.
 *   Status 4 of the scalars therefore also means a singular or non-finite diagonal block, found before the first iteration with x as given.
 * wlsqm_hip_krylov_block_start_device / _bicgstab_device: wlsqm_hip_krylov_start_device / _bicgstab_device with P taken from `planes` as
 *   the last factor left it (the start does not factor).  The P and S steps apply P in the launch that forms p and s
 *   ("krylov-update-block"), z_i = sum_j W[.., j, lane] * v_j with j ascending and fma; the other six launches of an iteration are the
 *   Jacobi route's own kernels.  For M^T pass the transposed matrix and the transposed plane.  The workspace is the same.
 * wlsqm_hip_krylov_block_precondition_device ("krylov-precondition", one launch): out = P v; v and out must not overlap.
 * WLSQM_EVALUE as above, and for a block other than 8, 16, 32. */
int64_t wlsqm_hip_krylov_block_bytes(int64_t nrows, int block);
int wlsqm_hip_krylov_block_factor_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                         const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                         int block, void* planes, void* planes_t, int device, void* stream);
int wlsqm_hip_krylov_block_start_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                        const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                        int block, const void* planes, const double* b, const double* x, double rtol, double atol,
                                        int64_t maxiter, void* workspace, int device, void* stream);
int wlsqm_hip_krylov_block_bicgstab_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                           const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                           int block, const void* planes, double* x, int64_t niter, void* workspace, int device,
                                           void* stream);
int wlsqm_hip_krylov_block_precondition_device(int64_t nrows, int block, const void* planes, const double* v, double* out, int device,
                                               void* stream);

/* ---- stacked right-hand sides of those solves (extension; csrc/krylov.hip) ----
 * nfields (1 .. 8) INDEPENDENT BiCGSTAB recurrences on the same M, one per field, in the launches of one: the matrix, and a block plane,
 * are read once per pass for all of them.  This is not a block Krylov method: every field has its own scalars, its own threshold
 * max(rtol * ||b_f||_2, atol) and its own stop, breakdown and non-finite checks, and the bits of field f — x, iterations, status, rr —
 * are those of the single-field functions above on b_f and x_f alone, with every preconditioner.  A field that has stopped is frozen:
 * no later launch writes its x or its scalars, while the others go on; a non-finite value in one field never reaches another.
 * b and x are (nfields, nrows) with any strides, element (f, i) at [f * stride_field + i * stride_point] (in doubles); the elements
 * of x must be distinct in memory.  precond: 0 none, 1 Jacobi, or 8 / 16 / 32: block-Jacobi with `planes` as
 * wlsqm_hip_krylov_block_factor_device left it (nslices must then be ceil(nrows / 64); `planes` is ignored otherwise).  Status 4
 * belongs to the matrix: it is set for every field before the first iteration, and x is untouched.
 * The workspace: wlsqm_hip_krylov_many_workspace_bytes(nrows, nfields) bytes, 16-byte aligned; the size depends on nfields only through
 * the pitch 2, 4 or 8 (the next one above nfields) at which the solver's own vectors are interleaved, v[i * pitch + f].  Its head is
 * 8 blocks of 128 bytes, the scalars of field 0 .. 7 in the layout above, then one int32 `done_all` (set when every field has stopped:
 * every kernel returns at its head then) in a block of 128 bytes: one read of 1152 bytes tells all.
 * Nothing but kernel launches on `stream` ("krylov-diag", "krylov-spmv-many", "krylov-update-many", "krylov-update-block-many",
 * "krylov-reduce-many"), as many as one single-field solve takes.  WLSQM_EVALUE as above, and for nfields outside 1 .. 8 or another precond.
 *
 * wlsqm_hip_krylov_many_start_device / _bicgstab_device: wlsqm_hip_krylov_start_device / _bicgstab_device for all fields.
 * wlsqm_hip_krylov_many_product_device: out_f = M in_f with dot0 = (out_f, w_f) and dot1 = (out_f, out_f) in the scalars of field f; in,
 *   w and out each with strides of their own; it has no preconditioner to name.  Not between a start and the end of its solve. */
int64_t wlsqm_hip_krylov_many_workspace_bytes(int64_t nrows, int nfields);
int wlsqm_hip_krylov_many_start_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                       const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                       int nfields, const double* b, int64_t b_stride_field, int64_t b_stride_point, const double* x,
                                       int64_t x_stride_field, int64_t x_stride_point, int precond, const void* planes, double rtol,
                                       double atol, int64_t maxiter, void* workspace, int device, void* stream);
int wlsqm_hip_krylov_many_bicgstab_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                          const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                          int nfields, double* x, int64_t x_stride_field, int64_t x_stride_point, int precond,
                                          const void* planes, int64_t niter, void* workspace, int device, void* stream);
int wlsqm_hip_krylov_many_product_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                         const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                         int nfields, const double* in, int64_t in_stride_field, int64_t in_stride_point, const double* w,
                                         int64_t w_stride_field, int64_t w_stride_point, double* out, int64_t out_stride_field,
                                         int64_t out_stride_point, void* workspace, int device, void* stream);

/* ---- BiCGSTAB(2) for the large steps where BiCGSTAB breaks down (extension; csrc/krylov.hip) ----
 * The same M x = b, right-preconditioned (A = M P; precond and `planes` as the _many_ functions take them: 0 none, 1 Jacobi, 8 / 16 / 32
 * the block plane of the last factor), by the method of Sleijpen and Fokkema with l = 2: two BiCG steps, then one residual minimisation
 * over span(A r, A^2 r), with rt the residual of the start:
 *   cycle:  rho0 = -omega rho0
 *     j = 0:  beta = alpha (rt, r) / rho0;  rho0 = (rt, r);  u = r - beta u;  u1 = A u;  alpha = rho0 / (rt, u1);  r -= alpha u1;  r1 = A r
 *     j = 1:  beta = alpha (rt, r1) / rho0; rho0 = (rt, r1); u = r - beta u, u1 = r1 - beta u1;  u2 = A u1;  alpha = rho0 / (rt, u2)
 *             r -= alpha u1, r1 -= alpha u2;  r2 = A r1
 *     MR:     s1 = (r1, r1), c1 = (r, r1), a12 = (r2, r1), a22 = (r2, r2), c2 = (r, r2);  tau = a12 / s1;  s2 = a22 - tau a12
 *             g2 = (c2 - tau c1) / s2;  g1 = c1 / s1 - tau g2;  omega = g2;  r -= g1 r1 + g2 r2;  u -= g1 u1 + g2 u2
 *             x += P (alpha_0 u_0 + alpha_1 u_1 + g1 r + g2 r1): the one place where x is written, behind every check of the cycle
 * A cycle is 4 products in 14 launches and counts as 2 iterations: `iterations`, `maxiter` and the scalars' layout are those of the
 * functions above (rho is the last (rt, r), rho_old the recurrence's rho0; beta, g1 and g2 follow the int32s as three doubles).  The stop
 * test, the iteration limit and `done` are taken at the end of a cycle, so a solve may pass an odd maxiter by one.  Status 2: rho0 == 0,
 * (rt, u1) == 0 or (rt, u2) == 0; 3: a non-finite dot product, alpha, beta or g; 4 as above, before the first cycle.  s1 == 0 takes
 * g1 = g2 = 0 and s2 == 0 takes g2 = 0, g1 = c1 / s1: omega is then 0 and the next cycle answers status 2 unless the solve has converged.
 * (rt, u2) == 0 waits in the same way: the cycle holds the step j = 0 by then, so it takes alpha = 0 and rho0 = 0, ends as ever (x receives
 * alpha_0 u_0 and the minimisation) and leaves status 2 to the next cycle's head; a system of one row converges through this rule.
 * A solve that stops on status 2 or 3 leaves x at the last finite iterate.  b == 0 with x == 0 converges at 0 iterations without a division.
 * The dot products are summed in the fixed order of the functions above, without atomics.
 * The workspace: wlsqm_hip_krylov_l2_workspace_bytes(nrows) bytes, 16-byte aligned: the 128 bytes of scalars, 5 planes of partial sums and
 * 10 vectors.  Nothing but kernel launches on `stream` ("krylov-diag", "krylov-spmv-dot", "krylov-l2-reduce", "krylov-l2-update",
 * "krylov-l2-update-block").  WLSQM_EVALUE as for the _many_ functions.
 *
 * wlsqm_hip_krylov_l2_start_device: wlsqm_hip_krylov_start_device for this method (at most 4 launches).
 * wlsqm_hip_krylov_l2_device: `ncycles` cycles behind a start with the same arguments.
 * wlsqm_hip_krylov_product_device and _grads_device serve this workspace too. */
int64_t wlsqm_hip_krylov_l2_workspace_bytes(int64_t nrows);
int wlsqm_hip_krylov_l2_start_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                     const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                     int precond, const void* planes, const double* b, const double* x, double rtol, double atol,
                                     int64_t maxiter, void* workspace, int device, void* stream);
int wlsqm_hip_krylov_l2_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                               const int32_t* col, const double* val, const double* diag, double diag_const, double scale, int precond,
                               const void* planes, double* x, int64_t ncycles, void* workspace, int device, void* stream);

/* ---- sparse approximate inverse preconditioner of those solves (extension; csrc/krylov.hip) ----
 * P = Q = diag(qd) + (the plane qv on the matrix's own SELL-64 structure): row i of Q minimises ||q^T M - e_i^T||_2 over the pattern
 * of row i of M, so Q M ~ I; the solves stay right-preconditioned (A = M Q).  The unknowns of row i are its slots: slot 0 the diagonal,
 * slot k the stored entry k - 1; a slot whose column an earlier slot names (the own entry of an F-known row, a neighbour named twice)
 * is dead and its coefficient is 0.0.  With J the columns of the live slots and m_r row r of M:
 *   G[a][b] = m_J[a] . m_J[b],  rhs[a] = (m_J[a])_i,  G q = rhs  by L D L^T without pivoting.
 * The planes: wlsqm_hip_krylov_spai_bytes(nrows, total) bytes of device memory, 8-byte aligned, `total` the matrix's stored entries:
 * qd (nrows doubles), the per-slice counts of the rows whose factorisation met a pivot that is not positive and finite
 * (ceil(nrows / 64) doubles; such a row of Q is zeros, and every start reduces the counts into status 4 with x untouched), then qv (total).
 *
 * wlsqm_hip_krylov_spai_build_device ("krylov-spai", one launch; a second with planes_t): Q from the matrix, diag and scale as they are on
 *   `stream`.  One wave per slice, its rows in turn; no atomics on anything that is summed, no scratch memory: the bits of Q are a function of
 *   the arguments.  An own entry (column r in row r) counts as part of the row's diagonal: a row is read as d_r plus its own entries in
 *   entry order, then its other entries.  max_width: the widest slice of the matrix, at most 65 (WLSQM_EVALUE above): 64 stored entries,
 *   or 65 where the 65th is the row's own entry (a row that stores anything else there fails: status 4).  planes_t (nullable): the planes of Q^T on
 *   the transposed structure, filled through npairs (dest, src) pairs of positions (transposed, forward) of the stored entries: the same
 *   numbers moved, not an approximate inverse of M^T.
 * wlsqm_hip_krylov_spai_apply_device ("krylov-spai-apply", one launch): out = Q v on the structure that the planes belong to (the forward
 *   one, or the transposed one with planes_t); v and out must not overlap.
 * wlsqm_hip_krylov_spai_start_device / _iterate_device: wlsqm_hip_krylov_start_device / _bicgstab_device (l2 == 0: `niter` iterations of
 *   10 launches, "krylov-spai-update": p and s by the update kernels, phat = Q p and shat = Q s by launches of their own) or
 *   wlsqm_hip_krylov_l2_start_device / _l2_device (l2 != 0: `niter` cycles of 19 launches, "krylov-spai-l2-update": Q applied 5 times, the
 *   last one adding to x between the cycle's last update and the reduce that takes the stop) with P = Q from `planes`; the workspaces are
 *   those methods' own, the matrix M or M^T with the planes of the same structure. */
int64_t wlsqm_hip_krylov_spai_bytes(int64_t nrows, int64_t total);
int wlsqm_hip_krylov_spai_build_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                       const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                       int max_width, void* planes, int64_t npairs, const int32_t* pair_dest, const int32_t* pair_src,
                                       void* planes_t, int device, void* stream);
int wlsqm_hip_krylov_spai_apply_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                       const int32_t* col, const void* planes, const double* v, double* out, int device, void* stream);
int wlsqm_hip_krylov_spai_start_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                       const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                       int l2, const void* planes, const double* b, const double* x, double rtol, double atol,
                                       int64_t maxiter, void* workspace, int device, void* stream);
int wlsqm_hip_krylov_spai_iterate_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                         const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                         int l2, const void* planes, double* x, int64_t niter, void* workspace, int device, void* stream);

/* ---- overlapping blocks: a restricted additive Schwarz preconditioner of those solves (extension; csrc/krylov.hip) ----
 * Block B is rows B * block .. B * block + block - 1 of M (block one of 8, 16, 32; the last block cut at nrows: cnt rows).  Its set ext_B
 * is those rows followed by at most rows - cnt others in ascending order (rows one of 32, 64, rows > block), which the caller chooses:
 *   table[B * rows + p]   int32   position p of ext_B, ceil(nrows / block) * rows of them on the device; -1: none.  The positions p < cnt
 *                                 are read as B * block + p whatever the table holds, and an entry outside 0 .. nrows - 1 or inside the
 *                                 block's own range counts as -1, so no table can make a kernel read out of bounds.  The entries
 *                                 behind the block's own must be ascending and distinct, the -1s last: the kernels find a column by
 *                                 a binary search of that list, and in a table that is not sorted an entry that the search misses
 *                                 is left out of A_B without an error (still a valid preconditioner, not the documented one).
 * A_B = M[ext_B, ext_B], entry (p, q) = d_ext[p] where ext[p] == ext[q], plus scale * (the sum of row ext[p]'s entries in column ext[q], in
 * entry order); a -1 position is an identity row and column.  P keeps the block's own rows of the exact inverse,
 *   z[B * block + i] = sum_q W_B[i][q] * v[ext_B[q]],  W_B the first cnt rows of A_B^-1,  q ascending with fma, 0.0 for v at a -1:
 * every row of z is written by one block (no scatter, no atomics), which is what "restricted" means.  The solves stay right-preconditioned.
 * The plane: wlsqm_hip_krylov_schwarz_bytes(nrows, block, rows) bytes of device memory, 8-byte aligned,
 *   W[(slice * rows + q) * 64 + lane]   float64   entry (lane % block, q) of W_B for the block that holds row slice * 64 + lane,
 * nslices * rows * 64 doubles, so that a wave reads column q of its slice as one contiguous run of 512 bytes; zeros in the rows beyond
 * nrows.  Behind them nslices * (64 / block) doubles, one per block position: 1.0 where the last build could not invert the block.
 *
 * wlsqm_hip_krylov_schwarz_build_device ("krylov-schwarz-build", one launch): one wave per block, lane p gathering row ext[p] from whatever
 *   slice holds it, then Gauss-Jordan elimination in LDS by the pivoting rule of wlsqm_hip_krylov_block_factor_device (the largest entry of
 *   the column among the rows not yet used, the lowest row at a tie).  planes_t (nullable): a second plane that receives the first cnt rows
 *   of (A_B^T)^-1 from the same elimination: the same preconditioner of M^T on the same sets (not P^T, whose application would scatter).
 *   A zero or non-finite pivot or a non-finite inverse counts the block as unusable: never a fault, and the next start answers status 4
 *   with x as given.  No scratch memory.
 * wlsqm_hip_krylov_schwarz_apply_device ("krylov-schwarz-apply", one launch): out = P v; a wave serves a slice, gathers v[ext[q]] of its
 *   64 / block blocks once into LDS and reads the plane column by column.  v and out must not overlap.
 * wlsqm_hip_krylov_schwarz_start_device / _iterate_device: wlsqm_hip_krylov_spai_start_device / _iterate_device with this P: l2 == 0,
 *   `niter` iterations of 10 launches ("krylov-schwarz-update"); l2 != 0, `niter` cycles of 19 launches ("krylov-schwarz-l2-update").  P is
 *   applied by launches of its own because a block reads rows that other workgroups of an update launch would still be writing.  For M^T
 *   pass the transposed matrix with the transposed plane and the same table.
 * WLSQM_EVALUE as above, and for another block or rows. */
int64_t wlsqm_hip_krylov_schwarz_bytes(int64_t nrows, int block, int rows);
int wlsqm_hip_krylov_schwarz_build_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                          const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                          int block, int rows, const int32_t* table, void* planes, void* planes_t, int device,
                                          void* stream);
int wlsqm_hip_krylov_schwarz_apply_device(int64_t nrows, int block, int rows, const int32_t* table, const void* planes, const double* v,
                                          double* out, int device, void* stream);
int wlsqm_hip_krylov_schwarz_start_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                          const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                          int l2, int block, int rows, const int32_t* table, const void* planes, const double* b,
                                          const double* x, double rtol, double atol, int64_t maxiter, void* workspace, int device,
                                          void* stream);
int wlsqm_hip_krylov_schwarz_iterate_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                            const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                            int l2, int block, int rows, const int32_t* table, const void* planes, double* x,
                                            int64_t niter, void* workspace, int device, void* stream);

/* ---- coupled fields: implicit solves with m unknowns per point (extension; csrc/krylov.hip) ----
 * BiCGSTAB on M x = b with block (a, b) of M = D_ab + sum_o coupling[a][b][o] * A_o, 1 <= m <= 4 unknowns per point, A_o the nop <= 8
 * value planes of a SQUARE matrix in the SELL-64 layout above (`val` points at plane 0, plane o at val + o * total).  coupling: HOST
 * array of m * m * nop doubles, [(a * m + b) * nop + o]; it travels to the kernels as an argument.  D_ab is a diagonal matrix:
 * diag != NULL: a device array (m, m, npoints), D_ab,i = diag[(a * m + b) * npoints + i]; else diag_const, a HOST array of m * m constants.
 * The unknowns, b and every product are interleaved: x[i * m + a] is component a at point i, so that a neighbour's unknowns are 8 m
 * contiguous bytes; for m = 2 and 4 they are moved by 16-byte loads, and b, x, in, w, out and the workspace must be 16-byte aligned
 * (WLSQM_EVALUE otherwise).  The product's order of operations is stated at the head of that part of csrc/krylov.hip.
 * jacobi != 0: right-preconditioned with the inverse of M's scalar diagonal, D_aa,i + sum_o coupling[a][a][o] * (the sum of row i's entries
 * in column i of plane o, in entry order), recomputed by every start.
 * The workspace, the scalars at its head, the statuses, the early exit on `done` and the fixed order of every sum are those of
 * wlsqm_hip_krylov_start_device at nrows = m * npoints: wlsqm_hip_krylov_system_workspace_bytes(npoints, m) is
 * wlsqm_hip_krylov_workspace_bytes(m * npoints) (-1 for m outside 1 .. 4).  Kernel launches only ("krylov-system-diag",
 * "krylov-system-spmv", "krylov-update", "krylov-reduce"): 4 for a start, 8 per iteration, 2 for a product.  WLSQM_EVALUE as there, and
 * for m outside 1 .. 4 or nop outside 1 .. 8. */
int64_t wlsqm_hip_krylov_system_workspace_bytes(int64_t npoints, int m);
int wlsqm_hip_krylov_system_start_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                         const int32_t* col, const double* val, int64_t total, int nop, int m, const double* coupling,
                                         const double* diag, const double* diag_const, int jacobi, const double* b, const double* x,
                                         double rtol, double atol, int64_t maxiter, void* workspace, int device, void* stream);
int wlsqm_hip_krylov_system_bicgstab_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                            const int32_t* col, const double* val, int64_t total, int nop, int m, const double* coupling,
                                            const double* diag, const double* diag_const, int jacobi, double* x, int64_t niter,
                                            void* workspace, int device, void* stream);
int wlsqm_hip_krylov_system_product_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                           const int32_t* col, const double* val, int64_t total, int nop, int m, const double* coupling,
                                           const double* diag, const double* diag_const, const double* in, const double* w, double* out,
                                           void* workspace, int device, void* stream);

/* ---- coupled fields: transposed solves and gradients (extension; csrc/krylov.hip) ----
 * The three calls above for M^T, whose block (a, b) is D_ba + sum_o coupling[b][a][o] * A_o^T: len .. val are the arrays of the TRANSPOSED
 * planes (total their stored entries), while coupling, diag and diag_const are the forward system's own, unchanged: the call exchanges
 * (a, b) in the host tables and reads a diag tensor in place at the exchanged index.  Everything else — workspace, scalars, statuses,
 * launches, alignment — is as above; the Jacobi diagonal holds the same numbers as the forward system's. */
int wlsqm_hip_krylov_system_start_transposed_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                                    const int64_t* soff, const int32_t* col, const double* val, int64_t total, int nop, int m,
                                                    const double* coupling, const double* diag, const double* diag_const, int jacobi,
                                                    const double* b, const double* x, double rtol, double atol, int64_t maxiter,
                                                    void* workspace, int device, void* stream);
int wlsqm_hip_krylov_system_bicgstab_transposed_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                                       const int64_t* soff, const int32_t* col, const double* val, int64_t total, int nop,
                                                       int m, const double* coupling, const double* diag, const double* diag_const,
                                                       int jacobi, double* x, int64_t niter, void* workspace, int device, void* stream);
int wlsqm_hip_krylov_system_product_transposed_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                                      const int64_t* soff, const int32_t* col, const double* val, int64_t total, int nop,
                                                      int m, const double* coupling, const double* diag, const double* diag_const,
                                                      const double* in, const double* w, double* out, void* workspace, int device,
                                                      void* stream);
/* The gradients of a loss L through M x = b from x and lam, the solution of M^T lam = dL/dx, both (npoints, m) interleaved, in one pass
 * over the FORWARD structure ("krylov-system-grads"; the values are not read):
 *   grad_val  (nop, total), the planes' layout, or NULL: dL/d(entry e of row j in plane o) = -sum_b (sum_a coupling[a][b][o] lam[j][a])
 *             x[col][b] at the live entries, +0.0 in every padding position;
 *   grad_diag (m, m, npoints) or NULL: -(lam[i][a] * x[i][b]).
 * The order of operations is stated at the head of the kernel.  One launch, no workspace, no atomics; lam and x 16-byte aligned for
 * m = 2 and 4.  WLSQM_EVALUE when neither output is asked for (total == 0 counts grad_val as not asked for, and then as nothing to do). */
int wlsqm_hip_krylov_system_grads_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                         const int32_t* col, int64_t total, int nop, int m, const double* coupling, const double* lam,
                                         const double* x, double* grad_val, double* grad_diag, int device, void* stream);

/* ---- coupled fields: a per-point coupling (extension; csrc/krylov.hip) ----
 * The calls above with `coupling` a DEVICE tensor (m, m, nop, npoints), plane-major like the diag tensor, read on the stream by every call:
 *   M[(i, a), (j, b)] = D_ab,i * delta_ij + sum_o coupling[a][b][o][i] * A_o[i, j]
 * (the equation of point i carries its own coefficients).  The order of operations differs from the constant table's and is stated at
 * the head of that part of csrc/krylov.hip.  transposed == 0: len .. val are the forward arrays and `mixed` is not looked at
 * ("krylov-system-diag-point", "krylov-system-spmv-point"; 4 launches for a start, 8 per iteration, 2 for a product).
 * transposed != 0: M^T; len .. val are the arrays of the TRANSPOSED planes, coupling, diag and diag_const the forward system's own, and
 * `mixed` is a device plane of nop * m * npoints doubles, 16-byte aligned, that "krylov-system-mix" writes in front of every product of
 * "krylov-system-spmv-mixed" (5 launches for a start, 10 per iteration, 3 for a product).  Workspace, scalars, statuses, alignment
 * and WLSQM_EVALUE are those of the calls above.  wlsqm_hip_krylov_system_point_grads_device is wlsqm_hip_krylov_system_grads_device
 * with sum_a coupling[a][b][o][j] lam[j][a] for row j. */
int wlsqm_hip_krylov_system_point_start_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                               const int32_t* col, const double* val, int64_t total, int nop, int m, const double* coupling,
                                               const double* diag, const double* diag_const, int transposed, double* mixed, int jacobi,
                                               const double* b, const double* x, double rtol, double atol, int64_t maxiter, void* workspace,
                                               int device, void* stream);
int wlsqm_hip_krylov_system_point_bicgstab_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                                  const int64_t* soff, const int32_t* col, const double* val, int64_t total, int nop, int m,
                                                  const double* coupling, const double* diag, const double* diag_const, int transposed,
                                                  double* mixed, int jacobi, double* x, int64_t niter, void* workspace, int device,
                                                  void* stream);
int wlsqm_hip_krylov_system_point_product_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                                 const int64_t* soff, const int32_t* col, const double* val, int64_t total, int nop, int m,
                                                 const double* coupling, const double* diag, const double* diag_const, int transposed,
                                                 double* mixed, const double* in, const double* w, double* out, void* workspace, int device,
                                                 void* stream);
int wlsqm_hip_krylov_system_point_grads_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                               const int32_t* col, int64_t total, int nop, int m, const double* coupling, const double* lam,
                                               const double* x, double* grad_val, double* grad_diag, int device, void* stream);

/* ---- coupled fields: block-Jacobi over points (extension; csrc/krylov.hip) ----
 * P = blockdiag(M_BB)^-1, block B the `points` consecutive points B points .. (B + 1) points - 1 with all m unknowns of each:
 * R = m * points <= 32 consecutive rows of the flat (npoints, m) vectors, the last block cut at npoints and completed by the identity.
 * The plane: wlsqm_hip_krylov_system_block_bytes(npoints, m, points) bytes of device memory (-1 for arguments out of range), 8-byte
 * aligned, 16-byte aligned for m = 2 and 4.  With NB the smallest of 8, 16, 32 that holds R and G = 64 / NB, lane g NB + l of wave w is
 * row l of block w G + g, and W[(w NB + j) 64 + lane] is entry (l, j) of that block's inverse; rows and columns from R on hold the
 * identity.  ceil(nwaves / 4) doubles behind the nwaves NB 64 count the unusable blocks of the last factor.
 * wlsqm_hip_krylov_system_block_factor_device ("krylov-system-blocks", one launch): len .. val are the FORWARD arrays, `coupling` the
 * host table (point == 0) or the device tensor (m, m, nop, npoints) (point != 0); `planes` receives the inverses and `planes_t`
 * (nullable) their transposes, which are the inverse blocks of M^T.  A block with a zero or non-finite pivot or a non-finite inverse
 * is counted, and the next start ends with status 4 before the first iteration.
 * wlsqm_hip_krylov_system_block_gather_device is an internal check hook, not part of the supported surface (the tests read the
 * gathered entries through it; it may change or go without notice): the same launch without the elimination; `planes` (of the same
 * size) receives the gathered blocks of M themselves in the same layout, identity padding included, and nothing is counted.
 * wlsqm_hip_krylov_system_block_precondition_device ("krylov-system-precondition", one launch): out = P v; v and out must not overlap.
 * The start and bicgstab forms are their siblings above with `points, planes` in the place of `jacobi`: the start reduces the plane's
 * counts where the sibling computes the scalar diagonal, and an iteration applies P in "krylov-system-update-block" (8 launches, 10 on
 * the per-point transposed route).  The transposed forms take the arrays of the transposed planes and the plane of the transposes.
 * WLSQM_EVALUE before any launch: points < 1 or m * points > 32, a null plane, a plane that is not 16-byte aligned for m = 2 or 4, and
 * what the siblings refuse. */
int64_t wlsqm_hip_krylov_system_block_bytes(int64_t npoints, int m, int points);
int wlsqm_hip_krylov_system_block_factor_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                                const int64_t* soff, const int32_t* col, const double* val, int64_t total, int nop, int m,
                                                const double* coupling, const double* diag, const double* diag_const, int point, int points,
                                                void* planes, void* planes_t, int device, void* stream);
int wlsqm_hip_krylov_system_block_gather_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                                const int64_t* soff, const int32_t* col, const double* val, int64_t total, int nop, int m,
                                                const double* coupling, const double* diag, const double* diag_const, int point, int points,
                                                void* planes, int device, void* stream);
int wlsqm_hip_krylov_system_block_precondition_device(int64_t npoints, int m, int points, const void* planes, const double* v, double* out,
                                                      int device, void* stream);
int wlsqm_hip_krylov_system_block_start_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                               const int32_t* col, const double* val, int64_t total, int nop, int m, const double* coupling,
                                               const double* diag, const double* diag_const, int points, const void* planes, const double* b,
                                               const double* x, double rtol, double atol, int64_t maxiter, void* workspace, int device,
                                               void* stream);
int wlsqm_hip_krylov_system_block_bicgstab_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                                  const int64_t* soff, const int32_t* col, const double* val, int64_t total, int nop, int m,
                                                  const double* coupling, const double* diag, const double* diag_const, int points,
                                                  const void* planes, double* x, int64_t niter, void* workspace, int device, void* stream);
int wlsqm_hip_krylov_system_block_start_transposed_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                                          const int64_t* soff, const int32_t* col, const double* val, int64_t total, int nop,
                                                          int m, const double* coupling, const double* diag, const double* diag_const,
                                                          int points, const void* planes, const double* b, const double* x, double rtol,
                                                          double atol, int64_t maxiter, void* workspace, int device, void* stream);
int wlsqm_hip_krylov_system_block_bicgstab_transposed_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                                             const int64_t* soff, const int32_t* col, const double* val, int64_t total,
                                                             int nop, int m, const double* coupling, const double* diag,
                                                             const double* diag_const, int points, const void* planes, double* x,
                                                             int64_t niter, void* workspace, int device, void* stream);
int wlsqm_hip_krylov_system_point_block_start_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                                     const int64_t* soff, const int32_t* col, const double* val, int64_t total, int nop, int m,
                                                     const double* coupling, const double* diag, const double* diag_const, int transposed,
                                                     double* mixed, int points, const void* planes, const double* b, const double* x,
                                                     double rtol, double atol, int64_t maxiter, void* workspace, int device, void* stream);
int wlsqm_hip_krylov_system_point_block_bicgstab_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                                        const int64_t* soff, const int32_t* col, const double* val, int64_t total, int nop,
                                                        int m, const double* coupling, const double* diag, const double* diag_const,
                                                        int transposed, double* mixed, int points, const void* planes, double* x,
                                                        int64_t niter, void* workspace, int device, void* stream);

/* ---- measurement hooks used by bench.py (not part of the reference surface) ---- */
/* Runs `reps` back-to-back launches of the fit kernel for batch `b` (device-resident, uniform
 * order) on `stream`, bracketed by HIP events on that stream; returns the mean kernel time in
 * milliseconds in *ms_out. */
int wlsqm_hip_time_fit_device(const wlsqm_batch* b, int device, void* stream, int order_uniform,
                              int reps, float* ms_out);
/* Same for the index-based path (basic algorithm, no sensitivities). */
int wlsqm_hip_time_fit_cloud_device(int dimension, int order, int64_t ncases, int64_t max_nk,
                                    const double* S, const double* F, const int32_t* hoods, int64_t hoods_stride_case,
                                    const int32_t* point_index, const int32_t* nk, const int64_t* knowns,
                                    const int32_t* weighting_method, double* fi, int64_t fi_stride_case,
                                    int device, void* stream, int reps, float* ms_out);

#ifdef __cplusplus
}
#endif
#endif /* WLSQM_HIP_H */
