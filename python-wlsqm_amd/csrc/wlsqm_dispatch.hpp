// wlsqm_dispatch.hpp — what the host code AROUND the kernels shares (host only): the environment switches of the library and their
// readers, the layout test of the staged / tiled kernels' dense rows, the launch geometry of the persistent kernels, and the
// declaration of every function one translation unit defines and another calls.  No .hip file declares another file's function
// and none calls getenv: tests/test_abi_and_host.py::test_dispatch_header_is_the_one_place scans for both.
#pragma once
#include <cstdlib>

#include "wlsqm_internal.hpp"

namespace wlsqm {

// ---- environment switches ------------------------------------------------------------------------------------------------------
// EVERY switch the library reads, one row each: name, accepted values, effect.  USER rows are settings of a deployment (mirrored in
// INTEGRATION.md); A/B rows are measurement and test hooks that pick between kernels giving the same results (the tests and tools/
// flip them between calls inside one process: the readers below ask the environment on EVERY call, nothing is cached — except the
// two marked "first use").  "=c" compares the FIRST character of the value; unset or empty never matches.
//
//   name                             kind  values            effect
//   WLSQM_HIP_STRICT                 USER  0 | 1 | 2,a,A | 3,c,C   numerics mode of a thread at its first use: unset / empty / 0.. fast, 2.. / a.. / A.. accurate, 3.. / c.. / C.. contracted, anything else strict (api.hip; before the contracted mode existed, 3.. / c.. / C.. fell under "anything else")
//   WLSQM_HIP_REPACK_MB              USER  integer > 0       scratch of one slice of the repack / gather passes in MB (default 512; api.hip)
//   WLSQM_HIP_COPY_THREADS           USER  integer           host threads that pack rows for the host-array entry points (default 16, first use; hostio.hpp)
//   WLSQM_HIP_TRACE                  USER  present           the host-array fit prints its phase timings to stderr (api.hip)
//   WLSQM_HIP_SENS_SLICE_MB          USER  number > 0        scratch for the inverses of one slice of the sensitivities' path in MB (default 1024; fit_sens.hip)
//   WLSQM_HIP_MOMENT_CHUNK           USER  integer > 0       cases per chunk of the two-kernel 2D order-4 path (default 4M; fit_moment.hip)
//   WLSQM_HIP_DISABLE_TILE           A/B   =1                every launch on the generic kernels (lane, rows / wave): tiles_enabled()
//   WLSQM_HIP_DISABLE_REPACK         A/B   =1                no repack / gather into dense scratch rows in front of the tiled kernels: repack_enabled()
//   WLSQM_HIP_HOST_NK_ORDER          A/B   =0                the host entry points keep the caller's case order for ragged batches (api.hip)
//   WLSQM_HIP_GRID_MULT              A/B   number > 0        workgroups per resident slot of the persistent kernels (default 16): grid_multiple()
//   WLSQM_HIP_STAGE                  A/B   =0 | =a           dense basic fits: never / every covered shape on the staged kernel (fit_stage.hip)
//   WLSQM_HIP_STAGE_GATHER           A/B   =0 | =a           the same for index-based input (fit_stage.hip)
//   WLSQM_HIP_STAGE_RAGGED           A/B   =0                never the RAGGED copy of the staged kernel (fit_stage.hip)
//   WLSQM_HIP_STAGE_FORM             A/B   =t | =o           two waves per SIMD / one wave that owns its SIMD, whatever the order hint says (fit_stage.hip)
//   WLSQM_HIP_STAGE_DMA6             A/B   =0                dense 2D systems up to 6 unknowns, rows of whole 128-byte lines: the register-staged kernel instead of its LDS-DMA form (fit_stage.hip)
//   WLSQM_HIP_STAGE_INVERSE          A/B   =0                the inverses of dense 2D order 4 from the tile + moment-solve pair again (fit_stage.hip)
//   WLSQM_HIP_QUAD_SLICE             A/B   integer >= 64     cases per slice of the 3D order-4 moment workspace (tests: small slices; fit_stage.hip)
//   WLSQM_HIP_STAGE_REFINE           A/B   =0 | =a           refinement: never / every covered shape on the staged kernel (fit_stage_iter.hip)
//   WLSQM_HIP_STAGE_SENS             A/B   =a                sensitivities on the staged kernel (off unless "all"; =0 as well; fit_stage_iter.hip)
//   WLSQM_HIP_REFINE_RESIDENT_KB     A/B   integer           bound of the whole-rows-in-LDS form in KB, and by its PRESENCE: for every max_iter (fit_stage_iter.hip)
//   WLSQM_HIP_REFINE_WCACHE          A/B   =0 | =w | =f      no LDS cache beside the staging rows / the weights / the values (fit_stage_iter.hip)
//   WLSQM_HIP_REFINE_CACHE_KB        A/B   integer           LDS budget of that cache in KB (default 40; fit_stage_iter.hip)
//   WLSQM_HIP_REFINE_ROUNDS          A/B   =1                refinement in rounds over survivor lists (fit_tilek.hip; fit_stage_iter.hip then stands aside)
//   WLSQM_HIP_REFINE_DEBUG           A/B   present           print the survivors of each round (synchronises; fit_tilek.hip)
//   WLSQM_HIP_DISABLE_TILE_EXTRAS    A/B   =1                sensitivities / refinement not on the one-wave tile kernel (fit_tilek.hip)
//   WLSQM_TILEK_SHAPE                A/B   =1 | =4           the one-wave / four-wave runtime-K tile kernel first (fit_tilek.hip)
//   WLSQM_HIP_DISABLE_FIXEDK         A/B   =1                dense input skips the fixed-K tile tables (fit_tile.hip)
//   WLSQM_TILE_VARIANT               A/B   integer           tuning variant of the BASELINE shapes' tile / ring kernels (fit_tile.hip, fit_ring.hip)
//   WLSQM_HIP_TILE_RUN_STORE         A/B   =0                the fixed-K tile kernels store fi per lane instead of as the tile's run (wlsqm_tile.hpp)
//   WLSQM_HIP_DISABLE_RING           A/B   =1                no one-kernel ring fit (fit_ring.hip, fit_ring_gather.hip)
//   WLSQM_HIP_RING_TILES             A/B   integer >= 1      tiles per workgroup of the ring kernel (default 4), and by its PRESENCE: for 3D too (wlsqm_ring.hpp)
//   WLSQM_HIP_DISABLE_CHUNK_REFINE   A/B   =1                refinement of the 10- / 15-unknown systems not on the chunked kernel (fit_chunk.hip)
//   WLSQM_HIP_DISABLE_SENS_APPLY     A/B   =1                no inverse + MFMA path for sensitivities / refinement (fit_sens.hip)
//   WLSQM_HIP_SENS_NO_MOMENT         A/B   =1                2D order-4 inverses from the chunked kernel (fit_sens.hip)
//   WLSQM_HIP_SENS_WAVE              A/B   =1                3D order-3/4 inverses from fit_wave.hip instead of fit_rows.hip (fit_sens.hip)
//   WLSQM_HIP_SENS_GRID_MULT         A/B   number > 0        workgroups per resident slot of the apply kernel (default 2; fit_sens.hip)
//   WLSQM_HIP_DISABLE_ROWS           A/B   =1                3D orders 3-4 on fit_wave.hip instead of the row-per-lane kernel (fit_rows.hip)
//   WLSQM_ROWS_ONE_CASE              A/B   =1                one case per wave for 3D order 3 too (fit_rows.hip)
//   WLSQM_HIP_STRICT_NO_ROWS         A/B   =1                strict mode without its row-per-lane kernel (fit_strict.hip)
//   WLSQM_HIP_STRICT_NO_REG          A/B   =1                strict mode without its register kernel (fit_strict.hip)
//   WLSQM_HIP_ACCURATE_NO_STAGE      A/B   present           accurate mode: per-lane row loads for dense input too (fit_accurate.hip)
//   WLSQM_HIP_ACCURATE_NO_SPEC       A/B   =1                accurate mode: the two-pass form for every group (fit_accurate.hip)
//   WLSQM_HIP_SOLVE_MANY             A/B   =f | =o           the stacked solve on the FMA kernel / on the stored-operator MFMA kernel (expert.hip)
//   WLSQM_HIP_OP_WPG                 A/B   integer           waves per workgroup of the MFMA kernel (solve_op.hip)
//   WLSQM_HIP_OP_DEBUG               A/B   integer           experiments of that kernel: 1 no stores, 2 only the first block of fields loaded (solve_op.hip)
//   WLSQM_HIP_SOLVE_ADJOINT          A/B   =g | =o           the adjoint of the prepared solve: the geometric route (one fit adjoint per field) everywhere / the stored operator's transpose wherever it is eligible, whatever the stack size (expert.hip)
//   WLSQM_HIP_ADJOINT_FORM           A/B   =l | =r           the adjoint of the fit and its geometry adjoint: the lane form for every batch / the rows form wherever it is eligible, whatever measured faster for the shape (fit_adjoint.hip)

// first character of the value; '\0' when the switch is unset or empty
inline char env_first(const char* name) { const char* e = getenv(name); return e ? e[0] : '\0'; }
// set at all, to whatever
inline bool env_present(const char* name) { return getenv(name) != nullptr; }
// integer value into *v, which keeps the caller's default when the switch is unset; returns env_present(name)
inline bool env_int(const char* name, long long* v) { const char* e = getenv(name); if (e) *v = atoll(e); return e != nullptr; }
// the value when it is a number above zero, else `otherwise`
inline double env_positive(const char* name, double otherwise) {
    const char* e = getenv(name);
    const double v = e ? atof(e) : 0.0;
    return v > 0.0 ? v : otherwise;
}

inline bool tiles_enabled() { return env_first("WLSQM_HIP_DISABLE_TILE") != '1'; }
inline bool repack_enabled() { return tiles_enabled() && env_first("WLSQM_HIP_DISABLE_REPACK") != '1'; }

// ---- dense rows ----------------------------------------------------------------------------------------------------------------
// The part of "dense rows the staged / tiled kernels can take" that every such kernel shares: the rows of xk and fk contiguous at
// a pitch of K neighbour slots, both bases 16-byte aligned.  What ELSE a kernel needs (K even, or only K * dim; a least or largest
// K) differs from family to family and stands next to each call.
inline bool dense_rows(int dim, const KParams& p, long long K) {
    if (p.sxk_k != dim || p.sxk_j != K * dim || p.sfk_k != 1 || p.sfk_j != K) return false;
    return ((reinterpret_cast<uintptr_t>(p.xk) | reinterpret_cast<uintptr_t>(p.fk)) & 15u) == 0;
}

// ---- persistent launches -------------------------------------------------------------------------------------------------------
// Per-device launch facts of one persistent kernel (a process may drive several GPUs): CU count, the one-time opt-in to
// more than 64 KB of dynamic LDS, and (when the LDS size never changes) the workgroups that fit one CU.
struct KernelSetup { int cus[16] = {}; int per_cu[16] = {}; };

// Workgroups launched per resident workgroup slot.  A grid of exactly the resident workgroups leaves the tail of the launch
// unbalanced (1M C2 cases are 62 500 tiles over 3 072 waves: 20 or 21 tiles each, and the waves do not finish their tiles at
// the same pace); launching several workgroups per slot lets the dispatcher hand the leftovers to whichever slot frees up first
// (tools/tune.py g1 / g8 / g16 / g1000, interleaved: C2 0.1737 / 0.1665 / 0.1656 / 0.1655 ms, C5 0.3512 / 0.3426 / 0.3386 /
// 0.3409, C3 0.672 / 0.650 / 0.639).  WLSQM_HIP_GRID_MULT overrides it (A/B).
inline double grid_multiple() { return env_positive("WLSQM_HIP_GRID_MULT", 16.0); }

// Grid of a persistent launch: resident workgroups per CU x CUs of the current device x grid_multiple()
// (callers clamp it to the number of tiles).
inline int persistent_grid(const void* kern, int threads, size_t lds_bytes, size_t lds_optin, bool fixed_lds, KernelSetup& ks,
                           long long* grid) {
    int dev = 0;
    WLSQM_HIP_CHECK(hipGetDevice(&dev));
    if (dev < 0 || dev >= 16) { set_error("device ordinal out of range"); return WLSQM_EVALUE; }
    if (!ks.cus[dev]) {
        hipDeviceProp_t prop;
        WLSQM_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
        if (lds_optin > 64 * 1024)
            WLSQM_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_optin));
        ks.cus[dev] = prop.multiProcessorCount;
    }
    int occ = fixed_lds ? ks.per_cu[dev] : 0;
    if (!occ) {
        WLSQM_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, threads, lds_bytes));
        if (occ < 1) occ = 1;
        if (fixed_lds) ks.per_cu[dev] = occ;
    }
    *grid = (long long)((double)occ * ks.cus[dev] * grid_multiple());
    if (*grid < 1) *grid = 1;
    return WLSQM_OK;
}

// ---- the fit launchers ---------------------------------------------------------------------------------------------------------
// Launch the fit kernels for one (dimension, order) bucket (api.hip).  max_nk: extent of the neighbour axis (upper bound of nk[j]).
int launch_fit(int dimension, int order, const KParams& p, long long max_nk, hipStream_t stream);

// The families launch_fit offers a batch to, in its order.  One signature: K is the extent of the neighbour axis (p.max_nk);
// *handled = false with WLSQM_OK: not this family's batch, nothing was launched, the next one is asked.
using FitLauncher = int(int dimension, int order, const KParams& p, long long K, hipStream_t stream, bool* handled);
FitLauncher launch_fit_stage;                  // fit_stage.hip
FitLauncher launch_fit_stage_refine;           // fit_stage_iter.hip
FitLauncher launch_fit_ring;                   // fit_ring.hip
FitLauncher launch_fit_ring_gather;            // fit_ring_gather.hip
FitLauncher launch_fit_moment;                 // fit_moment.hip
FitLauncher launch_fit_tile;                   // fit_tile.hip, and its per-family tables:
FitLauncher launch_fit_tile_even;              //   fit_tile_even.hip (dense, K <= 64)
FitLauncher launch_fit_tile_gather;            //   fit_tile_gather.hip (index-based)
FitLauncher launch_fit_tile_big;               //   fit_tile_big.hip (64 < K <= 128)
FitLauncher launch_fit_tilek;                  // fit_tilek.hip
FitLauncher launch_fit_sens;                   // fit_sens.hip
FitLauncher launch_fit_chunk_refine;           // fit_chunk.hip
FitLauncher launch_fit_chunk;                  // fit_chunk.hip
FitLauncher launch_fit_rows;                   // fit_rows.hip
FitLauncher launch_tile_moments;               // fit_tile.hip: first kernel of the two-kernel moment path (fit_moment.hip)
// the unconditional ends: every batch is theirs
int launch_fit_lane(int dimension, int order, const KParams& p, hipStream_t stream);                              // fit_lane.hip
int launch_fit_wave(int dimension, int order, const KParams& p, hipStream_t stream);                              // fit_wave.hip
int launch_fit_strict(int dimension, int order, const KParams& p, const StrictDebug* dbg, hipStream_t stream);    // fit_strict.hip
// accurate and contracted mode: offered every batch by launch_fit_strict before its own kernels (K is p.max_nk); FMA = contracted_mode()
template <bool FMA>
int launch_fit_accurate(int dimension, int order, const KParams& p, hipStream_t stream, bool* handled);           // fit_accurate.hip

// first kernels of the sensitivities' path (fit_sens.hip): the basic fit of one slice that also leaves every case's inverse normal matrix
bool chunk_inverse_ok(int dimension, int order, const KParams& p, long long K);                                   // fit_chunk.hip
int launch_fit_chunk_inverse(int dimension, int order, const KParams& p, long long K, hipStream_t stream);
bool moment_inverse_ok(int dimension, int order, const KParams& p, long long max_nk);                             // fit_moment.hip
int launch_fit_moment_inverse(int dimension, int order, const KParams& p, long long max_nk, double* inv, hipStream_t stream);
int launch_fit_stage_inverse(int dimension, int order, const KParams& p, long long K, double* inv, hipStream_t stream, bool* handled);   // fit_stage.hip
int launch_fit_rows_inverse(int dimension, int order, const KParams& p, double* inv, hipStream_t stream);         // fit_rows.hip
int launch_fit_wave_inverse(int dimension, int order, const KParams& p, double* inv, hipStream_t stream);         // fit_wave.hip

int launch_quad_solve(const KParams& p, hipStream_t stream);                                                      // fit_quad.hip: the solve behind fit_stage.hip's 3D order-4 moments

// The adjoint of the fit (fit_adjoint.hip): what it reads and writes beside the geometry in KParams (xk / hoods + S, nk, xi,
// knowns, wm, case_index; fk, fi and sens are not read).  g[j * sg_j + a] = dL/dfi_out; gfk[j * sgfk_j + k * sgfk_k] receives dL/dfk for
// every k < p.max_nk (zeros from nk[j] on); gfi[j * sgfi_j + a] (nullable: not wanted) receives dL/dfi_in and may alias g.
struct AdjointArgs {
    const double* g;   long long sg_j;
    double* gfk;       long long sgfk_j, sgfk_k;
    double* gfi;       long long sgfi_j;
};
// p.max_nk is the extent of the neighbour axis (set by the caller); 3D orders 3-4: WLSQM_EVALUE
int launch_fit_adjoint(int dimension, int order, const KParams& p, const AdjointArgs& q, hipStream_t stream);

// The geometry adjoint of the fit (fit_adjoint.hip): beside the geometry in KParams it READS the data (fk, or F through
// hoods) and the forward call's output p.fi (never written).  g as above; gxk[j * sgxk_j + k * sgxk_k + m] receives dL/dxk for every
// k < p.max_nk (zeros from nk[j] on), gxi[j * sgxi_j + m] dL/dxi, gfk (nullable: not wanted) dL/dfk as AdjointArgs::gfk.
struct GeometryAdjointArgs {
    const double* g;   long long sg_j;
    double* gxk;       long long sgxk_j, sgxk_k;
    double* gxi;       long long sgxi_j;
    double* gfk;       long long sgfk_j, sgfk_k;
};
// p.max_nk is the extent of the neighbour axis (set by the caller); 3D orders 3-4: WLSQM_EVALUE
int launch_fit_geometry_adjoint(int dimension, int order, const KParams& p, const GeometryAdjointArgs& q, hipStream_t stream);

// fit_tile.hip: the tile path's eligibility, for the families that share it
bool tile_dense_eligible(int dimension, const KParams& p, long long max_nk);                  // dense contiguous input the tile kernels can take
bool tile_moments_supported(int dimension, int order, const KParams& p, long long max_nk);    // 2D order 4 with a two-kernel moment instantiation (dense or index-based)
// Device row length (neighbour slots) for a batch whose largest neighbourhood has max_nk members: even, and for 2D order 4 at least 16
long long preferred_slots(int dimension, int order, long long max_nk);

// ---- behind wlsqm_expert (expert.hip) --------------------------------------------------------------------------------------------
int nearest_search(int dimension, int64_t ndata, const double* S, int64_t nquery, const double* X, int64_t x_stride,
                   long long* out, hipStream_t s);                                                                // knn.hip
int launch_solve_many(int dimension, int order, const KParams& p, long long K, long long nrhs,
                      const double* fk, long long sfk_r, long long sfk_j, double* fi, long long sfi_r, long long sfi_j,
                      hipStream_t stream, bool* handled);                                                         // solve_many.hip
int solve_op_build(int dimension, int order, const KParams& geom, long long K, const long long* h_knowns, long long ncases,
                   DevBuf& d_op, DevBuf& d_T, int* any_known, hipStream_t s, bool* ok);                           // solve_op.hip
int launch_solve_op(int dimension, int order, const KParams& geom, long long K, const double* op, const double* T, int any_known,
                    long long nrhs, const double* fk, long long sfk_r, long long sfk_j, double* fi, long long sfi_r, long long sfi_j,
                    hipStream_t stream, bool* handled);                                                           // solve_op.hip
bool solve_op_shape_ok(int dimension, int order, long long K);                                                     // solve_op.hip: shapes the stored operator covers
// The adjoint of R stacked fields through the stored operator's transpose: grad_fk[r][j][k] for k < min(gfk_slots,
// K rounded up to 8), grad_fi[r][j][a] for a < no (gfi nullable).  *handled = false with WLSQM_OK: not eligible, nothing was launched.
int launch_solve_op_adjoint(int dimension, int order, const KParams& geom, long long K, const double* op, const double* T, int any_known,
                            long long nrhs, const double* g, long long sg_r, long long sg_j, double* gfk, long long sgfk_r,
                            long long sgfk_j, long long gfk_slots, double* gfi, long long sgfi_r, long long sgfi_j, hipStream_t stream,
                            bool* handled);                                                                       // solve_op.hip
long long cond_workspace_doubles(int no);                                                                         // conds.hip
int launch_conds(int dimension, int order, const KParams& p, const int* order_arr, double* ws, long long CH,
                 long long case0, double* out, hipStream_t stream);                                               // conds.hip

}  // namespace wlsqm
