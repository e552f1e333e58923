// fit_adjoint.hip — the adjoint (vector-Jacobian product) of the WLSQM fit for gfx950 (wave64); DESIGN.md section 12.
//
// The fit is a linear map of its data: fi_U = M_UU^-1 (sum_k w_k fk_k c_{k,U} - M_{U,Kn} fi_Kn), U the unknowns, Kn the true knowns,
// D the DOFs dropped by stray high mask bits (effective_mask, wlsqm_kernels.hpp).  Given gbar = dL/dfi_out (n, no) the adjoint is
//   y_U = M_UU^-1 gbar_U (M is symmetric; y = 0 outside U),
//   grad_fk[k] = w_k (c_k . y) for k < nk and exactly 0 for nk <= k < K,
//   grad_fi[a] = gbar[a] - sum_k c_k[a] grad_fk[k] for a in Kn (= gbar[a] - (M y)[a]: no column of M has to survive the factorisation),
//                gbar[a] for a in D, 0 for a in U,
// and a case with every DOF known (the fit's no-op) has grad_fk = 0, grad_fi = gbar.  Neither fk nor the values in fi enter.
// One __device__ routine, adjoint_case, holds this arithmetic (the fast kernels': moment-free accumulate, FMA, LDL^T) and two kernels
// call it with their own row access, so a case's bits do not depend on the form that ran it:
//   "adjoint-lane": one lane per case, arbitrary strides, dense or index-based rows (the row access of fit_lane.hip), case_index;
//   "adjoint-rows": a wave owns 64 consecutive cases of dense rows: the lanes copy the wave's contiguous run of xk into LDS with 16-byte
//                   loads at an odd pitch, both passes read it from there (HBM is read once), grad_fk is written into the image
//                   (slot k * DIM of a row is dead once pass two has read neighbour k) and leaves as the wave's contiguous run.
#include "wlsqm_dispatch.hpp"
#include "wlsqm_kernels.hpp"

namespace wlsqm {

constexpr int ADJ_BLOCK = 64;                       // one wave per workgroup, as fit_lane.hip
constexpr size_t ADJ_LDS_BUDGET = 80 * 1024;        // per wave: at least two waves resident on a CU's 160 KiB

// Row access of the lane form: dense (xk rows with strides) or index-based (hoods row into S); grad_fk rows with strides.
template <int DIM>
struct AdjLaneRows {
    const double* xr; long long sxk_k;
    const int* hr; const double* S;                 // hr != nullptr: index-based
    double* out; long long sout_k;
    __device__ __forceinline__ void offset(int k, const double (&xi)[DIM], double (&d)[DIM]) const {
        const double* q = hr ? S + (long long)hr[k] * DIM : xr + k * sxk_k;
#pragma unroll
        for (int m = 0; m < DIM; ++m) d[m] = q[m] - xi[m];
    }
    __device__ __forceinline__ void put(int k, double v) const { out[k * sout_k] = v; }
};

// Row access of the rows form: the case's row of the wave's LDS image; grad_fk[k] overwrites the first coordinate of neighbour k.
template <int DIM>
struct AdjLdsRows {
    double* row;
    __device__ __forceinline__ void offset(int k, const double (&xi)[DIM], double (&d)[DIM]) const {
#pragma unroll
        for (int m = 0; m < DIM; ++m) d[m] = row[k * DIM + m] - xi[m];
    }
    __device__ __forceinline__ void put(int k, double v) const { row[k * DIM] = v; }
};

// M += w c c^T (upper triangle): accumulate() of wlsqm_kernels.hpp without its right-hand side, the fused operation spelled out
template <int N>
__device__ __forceinline__ void accumulate_matrix(double (&M)[N * (N + 1) / 2], const double (&c)[N], double w) {
    double t[N];
#pragma unroll
    for (int a = 0; a < N; ++a) t[a] = (a == 0) ? w : w * c[a];   // c[0] == 1
#pragma unroll
    for (int b = 0; b < N; ++b) M[tri<N>(0, b)] += t[b];
#pragma unroll
    for (int a = 1; a < N; ++a)
#pragma unroll
        for (int b = a; b < N; ++b) M[tri<N>(a, b)] = fma(t[a], c[b], M[tri<N>(a, b)]);
}

// The adjoint of one case.  grow: the case's gbar row (read in full before anything is written: it may alias gfi); gfi: nullable.
// K: neighbour slots of the row (nk <= K); rows.put(k, .) receives grad_fk[k] for every k < K.
template <int DIM, int ORDER, class Rows>
__device__ __forceinline__ void adjoint_case(const Rows& rows, const double (&xi)[DIM], int nk, int K, bool uniform,
                                             unsigned long long known, unsigned long long dropped, const double* grow, double* gfi) {
    constexpr int NO = ndofs(DIM, ORDER);
    constexpr int NE = NO * (NO + 1) / 2;
    constexpr unsigned long long FULL = (1ull << NO) - 1ull;
    double gb[NO], y[NO];
#pragma unroll
    for (int a = 0; a < NO; ++a) { gb[a] = grow[a]; y[a] = gb[a]; }
    if (known == FULL) {                            // nothing to solve: the fit leaves fi as it came in
        for (int k = 0; k < K; ++k) rows.put(k, 0.0);
        if (gfi) {
#pragma unroll
            for (int a = 0; a < NO; ++a) gfi[a] = gb[a];
        }
        return;
    }
    // pass 1: largest squared distance; not needed for uniform weights
    double max_d2 = 0.0;
    if (!uniform) {
        for (int k = 0; k < nk; ++k) {
            double d[DIM];
            rows.offset(k, xi, d);
            double d2 = d[0] * d[0];
            if constexpr (DIM >= 2) d2 += d[1] * d[1];
            if constexpr (DIM == 3) d2 += d[2] * d[2];
            if (d2 > max_d2) max_d2 = d2;
        }
    }
    const double inv_max = inverse_max(max_d2);
    // pass 2: M = C^T W C (upper triangle)
    double M[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) M[e] = 0.0;
    for (int k = 0; k < nk; ++k) {
        double d[DIM], c[NO];
        rows.offset(k, xi, d);
        const double d2 = monomials<DIM, ORDER>(d, c);
        accumulate_matrix<NO>(M, c, weight(d2, inv_max, uniform));
    }
    // knowns: rows and columns masked to identity, their entries of the right-hand side zeroed (the values are zero: nothing moves)
    {
        double zero[NO];
#pragma unroll
        for (int a = 0; a < NO; ++a) zero[a] = 0.0;
        eliminate_knowns<NO>(M, y, known, zero);
    }
    ldlt_factor<NO>(M);
    ldlt_solve<NO>(M, y);                           // y_U = M_UU^-1 gbar_U, y = 0 outside U
    // pass 3: grad_fk[k] = w_k (c_k . y); the true knowns' columns collect sum_k c_k[a] grad_fk[k] = (M y)[a]
    const bool sums = gfi != nullptr && (known & ~dropped) != 0ull;
    double acc[NO];
#pragma unroll
    for (int a = 0; a < NO; ++a) acc[a] = 0.0;
    for (int k = 0; k < nk; ++k) {
        double d[DIM], c[NO];
        rows.offset(k, xi, d);
        const double d2 = monomials<DIM, ORDER>(d, c);
        const double w = weight(d2, inv_max, uniform);
        double s = y[0];
#pragma unroll
        for (int a = 1; a < NO; ++a) s = fma(c[a], y[a], s);
        const double gk = w * s;
        rows.put(k, gk);
        if (sums) {
            acc[0] += gk;
#pragma unroll
            for (int a = 1; a < NO; ++a) acc[a] = fma(c[a], gk, acc[a]);
        }
    }
    for (int k = nk; k < K; ++k) rows.put(k, 0.0);  // the padding of a ragged row: exact zeros
    if (gfi) {
#pragma unroll
        for (int a = 0; a < NO; ++a) {
            double v = 0.0;                                          // an unknown's incoming value is never read by the fit
            if ((known >> a) & 1ull) v = ((dropped >> a) & 1ull) ? gb[a] : gb[a] - acc[a];
            gfi[a] = v;
        }
    }
}

template <int DIM, int ORDER>
__global__ __launch_bounds__(ADJ_BLOCK) void adjoint_lane_kernel(const KParams p, const AdjointArgs q) {
    constexpr int NO = ndofs(DIM, ORDER);
    const long long t = (long long)blockIdx.x * ADJ_BLOCK + threadIdx.x;
    if (t >= live_cases(p)) return;
    const long long j = p.case_index ? p.case_index[t] : t;
    const int K = (int)p.max_nk;
    const int nk = max(min(p.nk[j * p.snk], K), 0);                   // never past the end of a row
    const bool uniform = (p.wm[j * p.swm] == WLSQM_WEIGHT_UNIFORM);
    unsigned long long known, dropped;
    effective_mask<NO>(p.knowns[j * p.sknowns], known, dropped);
    double xi[DIM];
    AdjLaneRows<DIM> rows;
    double* out = q.gfk + j * q.sgfk_j;
    if (p.hoods) {
        const long long pj = own_point(p, j);
#pragma unroll
        for (int m = 0; m < DIM; ++m) xi[m] = p.S[pj * DIM + m];
        rows = AdjLaneRows<DIM>{nullptr, 0, p.hoods + j * p.shoods_j, p.S, out, q.sgfk_k};
    } else {
#pragma unroll
        for (int m = 0; m < DIM; ++m) xi[m] = p.xi[j * p.sxi_j + m];
        rows = AdjLaneRows<DIM>{p.xk + j * p.sxk_j, p.sxk_k, nullptr, nullptr, out, q.sgfk_k};
    }
    adjoint_case<DIM, ORDER>(rows, xi, nk, K, uniform, known, dropped, q.g + j * q.sg_j, q.gfi ? q.gfi + j * q.sgfi_j : nullptr);
}

// Copies between the wave's contiguous global run of `rows` rows of `len` doubles and its LDS image (row r at r * pitch, element e of
// a global row at LDS offset e * step).  16-byte pieces, a lane's position (row, element) advanced without a division per piece; a run of
// an odd number of doubles (odd len and odd rows) ends in one 8-byte piece.  The run's base is 16-byte aligned: the launcher checked the
// buffer's base, and a wave's offset into it is 64 rows.
template <bool TO_LDS>
__device__ __forceinline__ void adjoint_copy_run(double* lds, int pitch, int step, double* run, int rows, int len) {
    const int total = rows * len;                                    // doubles; at most 64 rows of an image below ADJ_LDS_BUDGET
    const int pairs = total >> 1;
    const int lane = threadIdx.x;
    int r = (2 * lane) / len, e = (2 * lane) % len;
    const int qs = (2 * ADJ_BLOCK) / len, rs = (2 * ADJ_BLOCK) % len;
    double2* run2 = reinterpret_cast<double2*>(run);
#pragma unroll 4
    for (int i = lane; i < pairs; i += ADJ_BLOCK) {
        int r1 = r, e1 = e + 1;
        if (e1 == len) { e1 = 0; ++r1; }
        if constexpr (TO_LDS) {
            const double2 v = run2[i];
            lds[r * pitch + e * step] = v.x;
            lds[r1 * pitch + e1 * step] = v.y;
        } else {
            double2 v;
            v.x = lds[r * pitch + e * step];
            v.y = lds[r1 * pitch + e1 * step];
            run2[i] = v;
        }
        e += rs; r += qs;
        if (e >= len) { e -= len; ++r; }
    }
    if ((total & 1) && lane == 0) {
        const int i = total - 1;
        if constexpr (TO_LDS) lds[(i / len) * pitch + (i % len) * step] = run[i];
        else run[i] = lds[(i / len) * pitch + (i % len) * step];
    }
}

template <int DIM, int ORDER>
__global__ __launch_bounds__(ADJ_BLOCK) void adjoint_rows_kernel(const KParams p, const AdjointArgs q, int pitch) {
    constexpr int NO = ndofs(DIM, ORDER);
    extern __shared__ double adj_lds[];
    const long long j0 = (long long)blockIdx.x * ADJ_BLOCK;
    const int K = (int)p.max_nk;
    const long long left = p.ncases - j0;
    const int ncw = left < ADJ_BLOCK ? (int)left : ADJ_BLOCK;          // the tail group has fewer than 64 cases
    adjoint_copy_run<true>(adj_lds, pitch, 1, const_cast<double*>(p.xk) + j0 * K * DIM, ncw, K * DIM);
    __syncthreads();
    if ((int)threadIdx.x < ncw) {
        const long long j = j0 + threadIdx.x;
        const int nk = max(min(p.nk[j * p.snk], K), 0);
        const bool uniform = (p.wm[j * p.swm] == WLSQM_WEIGHT_UNIFORM);
        unsigned long long known, dropped;
        effective_mask<NO>(p.knowns[j * p.sknowns], known, dropped);
        double xi[DIM];
#pragma unroll
        for (int m = 0; m < DIM; ++m) xi[m] = p.xi[j * p.sxi_j + m];
        const AdjLdsRows<DIM> rows{adj_lds + (int)threadIdx.x * pitch};
        adjoint_case<DIM, ORDER>(rows, xi, nk, K, uniform, known, dropped, q.g + j * q.sg_j, q.gfi ? q.gfi + j * q.sgfi_j : nullptr);
    }
    __syncthreads();
    adjoint_copy_run<false>(adj_lds, pitch, DIM, q.gfk + j0 * K, ncw, K);
}

// LDS pitch of a row of `len` doubles: odd, so that the 32 lanes of a ds_read_b64 lane group, one row each, hit 32 different bank pairs
static int adjoint_pitch(long long len) { return (int)(len | 1); }

// The rows form takes dense rows of xk and of grad_fk (dense_rows: contiguous at a pitch of K slots, bases 16-byte aligned), every
// case of the batch in order, and an image of 64 rows within the LDS budget.
static bool adjoint_rows_eligible(int dim, const KParams& p, const AdjointArgs& q, long long K) {
    if (p.hoods || p.case_index || p.ncases_dev || !p.xk || K < 1) return false;
    KParams t = p;
    t.fk = q.gfk; t.sfk_j = q.sgfk_j; t.sfk_k = q.sgfk_k;          // grad_fk has fk's layout
    if (!dense_rows(dim, t, K)) return false;
    return (size_t)adjoint_pitch(K * dim) * ADJ_BLOCK * sizeof(double) <= ADJ_LDS_BUDGET;
}

// Which form runs when WLSQM_HIP_ADJOINT_FORM is unset: the one that measured faster for the shape (1M cases, one
// MI355X, rows / lane): 2D order 2 at 32 neighbours 0.305 / 1.46 ms, 3D order 2 at 40 0.94 / 1.45, 1D order 2 at 8 (4M cases) 0.15 / 0.56,
// but 2D order 4 at 64 1.91 / 1.56: the 15-unknown system's 469 registers leave the rows form one wave per SIMD with nothing to hide
// its LDS latency behind, and the lane form's second and third passes find their rows in L2.  So: the systems up to 10 unknowns.
static bool adjoint_rows_default(int dimension, int order) {
    return wlsqm_hip_number_of_dofs(dimension, order) <= 10;
}

template <int DIM, int ORDER>
static int launch_adjoint(const KParams& p, const AdjointArgs& q, bool rows, hipStream_t stream) {
    const long long blocks = (p.ncases + ADJ_BLOCK - 1) / ADJ_BLOCK;
    if (blocks <= 0) return WLSQM_OK;
    if (blocks > 0x7fffffffLL) { set_error("too many cases for one launch"); return WLSQM_EVALUE; }
    if (rows) {
        const int pitch = adjoint_pitch(p.max_nk * DIM);
        const size_t lds = (size_t)pitch * ADJ_BLOCK * sizeof(double);
        if (lds > 64 * 1024) {                                       // the opt-in to more than 64 KiB of dynamic LDS, once per device
            static bool opted[16] = {};
            int dev = 0;
            WLSQM_HIP_CHECK(hipGetDevice(&dev));
            if (dev < 0 || dev >= 16) { set_error("device ordinal out of range"); return WLSQM_EVALUE; }
            if (!opted[dev]) {
                WLSQM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&adjoint_rows_kernel<DIM, ORDER>),
                                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)ADJ_LDS_BUDGET));
                opted[dev] = true;
            }
        }
        hipLaunchKernelGGL((adjoint_rows_kernel<DIM, ORDER>), dim3((unsigned)blocks), dim3(ADJ_BLOCK), lds, stream, p, q, pitch);
        WLSQM_HIP_CHECK(hipGetLastError());
        note_kernel("adjoint-rows");
        return WLSQM_OK;
    }
    hipLaunchKernelGGL((adjoint_lane_kernel<DIM, ORDER>), dim3((unsigned)blocks), dim3(ADJ_BLOCK), 0, stream, p, q);
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("adjoint-lane");
    return WLSQM_OK;
}

int launch_fit_adjoint(int dimension, int order, const KParams& p, const AdjointArgs& q, hipStream_t stream) {
    if (p.ncases <= 0) return WLSQM_OK;
    const char form = env_first("WLSQM_HIP_ADJOINT_FORM");          // =l: the lane form for everything; =r: the rows form wherever eligible
    const bool rows = form != 'l' && adjoint_rows_eligible(dimension, p, q, p.max_nk) && (form == 'r' || adjoint_rows_default(dimension, order));
#define CASE(D, O) if (dimension == D && order == O) return launch_adjoint<D, O>(p, q, rows, stream);
    CASE(1, 0) CASE(1, 1) CASE(1, 2) CASE(1, 3) CASE(1, 4)
    CASE(2, 0) CASE(2, 1) CASE(2, 2) CASE(2, 3) CASE(2, 4)
    CASE(3, 0) CASE(3, 1) CASE(3, 2)
#undef CASE
    set_error("fit_adjoint: unsupported (dimension, order)");
    return WLSQM_EVALUE;
}

// ---- the geometry adjoint: gradients with respect to the coordinates ------------------------------------------
// The fit is NOT linear in the offsets d_k = xk_k - xi.  With phi = fi_out (the entries in D replaced by 0), y as above, s_k = c_k . y,
// r_k = fk_k - c_k . phi and (d_m c)[a] the scaled monomial whose exponent on axis m is one lower (0 when that exponent is 0: it is
// another entry of c, Lowered below), the gradient of L = gbar . fi_out is, for k < nk,
//   e[k][m] = (dw_k/dd_k,m) s_k r_k + w_k (r_k (d_m c_k . y) - s_k (d_m c_k . phi)),
// dw = 0 under uniform weights, else with beta = 1 - 1e-4, D2 = max_k d2_k, rho_k = sqrt(d2_k / D2), t_k = 1 - rho_k
//   dw_k/dd_k,m = -2 beta t_k d_k,m / (rho_k D2)     (0 where rho_k == 0: the cone of |d| at d = 0 contributes nothing),
//   E = sum_k (beta t_k rho_k / D2) s_k r_k,   e[k*][m] += 2 d_k*,m E,   k* the SMALLEST index that attains D2 (pass 1's strict `>`:
//   a tie for the farthest neighbour goes to the smaller index),
// grad_xk[k][m] = e[k][m] (exact zeros for nk <= k < K), grad_xi[m] = -sum_k e[k][m], and, at no extra cost, grad_fk[k] = w_k s_k: the
// bits of adjoint_case's for the systems up to 10 unknowns (the same statements in the same order).  A case with every DOF known has
// zeros everywhere.  Three passes over the neighbours: D2 and k*; M, its factorisation and y (adjoint_solve); the loop above, which
// accumulates E and the xi sum and keeps d_k* and e[k*] in registers for the fix-up of slot k*.  Two kernels call it, as for the adjoint:
//   "geometry-adjoint-lane": one lane per case, arbitrary strides, dense or index-based rows, case_index;
//   "geometry-adjoint-rows": the wave's run of xk in LDS at the odd pitch, grad_xk[k] overwrites neighbour k's DIM coordinates in place
//                            and the image leaves as one contiguous run; fk is read once: through the image too where a row of
//                            K (DIM + 1) doubles fits the LDS budget (grad_fk then leaves as a run as well), else by each lane from its
//                            own global row.

// Pass two of adjoint_case, statement for statement (that routine is left as it was, so that its kernels compile to the code they had):
// M = C^T W C (upper triangle), the knowns masked out, the factorisation, and y (gbar on entry) overwritten with y_U = M_UU^-1 gbar_U,
// y = 0 outside U.
template <int DIM, int ORDER, class Rows>
__device__ __forceinline__ void adjoint_solve(const Rows& rows, const double (&xi)[DIM], int nk, bool uniform, double inv_max,
                                              unsigned long long known, double (&y)[ndofs(DIM, ORDER)]) {
    constexpr int NO = ndofs(DIM, ORDER);
    constexpr int NE = NO * (NO + 1) / 2;
    double M[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) M[e] = 0.0;
    for (int k = 0; k < nk; ++k) {
        double d[DIM], c[NO];
        rows.offset(k, xi, d);
        const double d2 = monomials<DIM, ORDER>(d, c);
        accumulate_matrix<NO>(M, c, weight(d2, inv_max, uniform));
    }
    // knowns: rows and columns masked to identity, their entries of the right-hand side zeroed (the values are zero: nothing moves)
    {
        double zero[NO];
#pragma unroll
        for (int a = 0; a < NO; ++a) zero[a] = 0.0;
        eliminate_knowns<NO>(M, y, known, zero);
    }
    ldlt_factor<NO>(M);
    ldlt_solve<NO>(M, y);
}

// low.idx[m][a]: the DOF whose exponent on axis m is one lower than DOF a's, -1 where that exponent is 0
template <int DIM, int ORDER>
struct Lowered {
    int idx[DIM][ndofs(DIM, ORDER)];
    constexpr Lowered() : idx{} {
        constexpr int NO = ndofs(DIM, ORDER);
        for (int m = 0; m < DIM; ++m)
            for (int a = 0; a < NO; ++a) {
                const int p = Mono<DIM>::P[a] - (m == 0), q = Mono<DIM>::Q[a] - (m == 1), r = Mono<DIM>::R[a] - (m == 2);
                idx[m][a] = -1;
                for (int b = 0; b < NO; ++b)
                    if (Mono<DIM>::P[b] == p && Mono<DIM>::Q[b] == q && Mono<DIM>::R[b] == r) idx[m][a] = b;
            }
    }
};

// Row access of the lane form: AdjLaneRows plus the data (fk rows with strides, or F through the hoods row) and the two outputs.
template <int DIM>
struct GeoLaneRows {
    const double* xr; long long sxk_k;
    const int* hr; const double* S;                 // hr != nullptr: index-based
    const double* fr; long long sfk_k; const double* F;
    double* out; long long sout_k;                  // grad_xk: DIM contiguous doubles per slot
    double* gfk; long long sgfk_k;                  // nullable
    __device__ __forceinline__ void offset(int k, const double (&xi)[DIM], double (&d)[DIM]) const {
        const double* q = hr ? S + (long long)hr[k] * DIM : xr + k * sxk_k;
#pragma unroll
        for (int m = 0; m < DIM; ++m) d[m] = q[m] - xi[m];
    }
    __device__ __forceinline__ double value(int k) const { return hr ? F[hr[k]] : fr[k * sfk_k]; }
    __device__ __forceinline__ void put(int k, const double (&e)[DIM]) const {
#pragma unroll
        for (int m = 0; m < DIM; ++m) out[k * sout_k + m] = e[m];
    }
    __device__ __forceinline__ void put_fk(int k, double v) const { if (gfk) gfk[k * sgfk_k] = v; }
};

// Row access of the rows form: the case's row of the wave's LDS image, overwritten slot by slot; fk and grad_fk in global memory.
template <int DIM>
struct GeoLdsRows {
    double* row;
    const double* fr; long long sfk_k;
    double* gfk; long long sgfk_k;                  // nullable
    __device__ __forceinline__ void offset(int k, const double (&xi)[DIM], double (&d)[DIM]) const {
#pragma unroll
        for (int m = 0; m < DIM; ++m) d[m] = row[k * DIM + m] - xi[m];
    }
    __device__ __forceinline__ double value(int k) const { return fr[k * sfk_k]; }
    __device__ __forceinline__ void put(int k, const double (&e)[DIM]) const {
#pragma unroll
        for (int m = 0; m < DIM; ++m) row[k * DIM + m] = e[m];
    }
    __device__ __forceinline__ void put_fk(int k, double v) const { if (gfk) gfk[k * sgfk_k] = v; }
};

// The geometry adjoint of one case.  grow: the case's gbar row; firow: the forward call's output row (read, never written); gxi: DIM doubles.
template <int DIM, int ORDER, class Rows>
__device__ __forceinline__ void geometry_adjoint_case(const Rows& rows, const double (&xi)[DIM], int nk, int K, bool uniform,
                                                      unsigned long long known, unsigned long long dropped, const double* grow,
                                                      const double* firow, double* gxi) {
    constexpr int NO = ndofs(DIM, ORDER);
    constexpr unsigned long long FULL = (1ull << NO) - 1ull;
    constexpr Lowered<DIM, ORDER> low{};
    constexpr double BETA = 1.0 - 1e-4;
    double zeros[DIM];
#pragma unroll
    for (int m = 0; m < DIM; ++m) zeros[m] = 0.0;
    if (known == FULL) {                            // nothing to solve: fi_out does not depend on the geometry
        for (int k = 0; k < K; ++k) { rows.put(k, zeros); rows.put_fk(k, 0.0); }
#pragma unroll
        for (int m = 0; m < DIM; ++m) gxi[m] = 0.0;
        return;
    }
    double y[NO];
#pragma unroll
    for (int a = 0; a < NO; ++a) y[a] = grow[a];
    // pass 1: largest squared distance and the first neighbour that attains it; not needed for uniform weights
    double max_d2 = 0.0;
    int kstar = -1;
    if (!uniform) {
        for (int k = 0; k < nk; ++k) {
            double d[DIM];
            rows.offset(k, xi, d);
            double d2 = d[0] * d[0];
            if constexpr (DIM >= 2) d2 += d[1] * d[1];
            if constexpr (DIM == 3) d2 += d[2] * d[2];
            if (d2 > max_d2) { max_d2 = d2; kstar = k; }
        }
    }
    const double inv_max = inverse_max(max_d2);
    // pass 2: M = C^T W C, its factorisation and y_U = M_UU^-1 gbar_U, y = 0 outside U
    adjoint_solve<DIM, ORDER>(rows, xi, nk, uniform, inv_max, known, y);
    double phi[NO];
#pragma unroll
    for (int a = 0; a < NO; ++a) phi[a] = ((dropped >> a) & 1ull) ? 0.0 : firow[a];
    // pass 3: e[k][m] per neighbour; E, the xi sum, and slot k*'s offset and gradient kept for the fix-up
    double E = 0.0, sum[DIM], dstar[DIM], estar[DIM];
#pragma unroll
    for (int m = 0; m < DIM; ++m) { sum[m] = 0.0; dstar[m] = 0.0; estar[m] = 0.0; }
    for (int k = 0; k < nk; ++k) {
        double d[DIM], c[NO], e[DIM];
        rows.offset(k, xi, d);
        const double fkk = rows.value(k);           // before put_fk: in the rows form's image grad_fk[k] takes the place of fk[k]
        const double d2 = monomials<DIM, ORDER>(d, c);
        const double w = weight(d2, inv_max, uniform);
        double s = y[0];
#pragma unroll
        for (int a = 1; a < NO; ++a) s = fma(c[a], y[a], s);
        rows.put_fk(k, w * s);
        double cp = phi[0];
#pragma unroll
        for (int a = 1; a < NO; ++a) cp = fma(c[a], phi[a], cp);
        const double r = fkk - cp;
        const double sr = s * r;
        // the weight's own derivative: selects, not branches (uniform weights: inv_max is not finite, everything here is discarded)
        const double rho = sqrt_unit(d2 * inv_max);
        const double t = 1.0 - rho;
        const double bt = (BETA * t) * inv_max;
        const double dwc = (uniform || !(rho > 0.0)) ? 0.0 : (-2.0 * bt) * recip(rho);
        E = uniform ? 0.0 : fma(bt * rho, sr, E);
#pragma unroll
        for (int m = 0; m < DIM; ++m) {
            double dcy = 0.0, dcp = 0.0;
#pragma unroll
            for (int a = 1; a < NO; ++a) {
                if (low.idx[m][a] >= 0) {
                    dcy = fma(c[low.idx[m][a]], y[a], dcy);
                    dcp = fma(c[low.idx[m][a]], phi[a], dcp);
                }
            }
            e[m] = fma(w, fma(r, dcy, -(s * dcp)), (dwc * d[m]) * sr);
            sum[m] += e[m];
            if (k == kstar) { dstar[m] = d[m]; estar[m] = e[m]; }
        }
        rows.put(k, e);
    }
    for (int k = nk; k < K; ++k) { rows.put(k, zeros); rows.put_fk(k, 0.0); }     // the padding of a ragged row: exact zeros
    if (kstar >= 0) {                               // D2 moves with its own neighbour only
#pragma unroll
        for (int m = 0; m < DIM; ++m) {
            const double fix = (2.0 * dstar[m]) * E;
            estar[m] += fix;
            sum[m] += fix;
        }
        rows.put(kstar, estar);
    }
#pragma unroll
    for (int m = 0; m < DIM; ++m) gxi[m] = -sum[m];
}

template <int DIM, int ORDER>
__global__ __launch_bounds__(ADJ_BLOCK) void geometry_adjoint_lane_kernel(const KParams p, const GeometryAdjointArgs q) {
    constexpr int NO = ndofs(DIM, ORDER);
    const long long t = (long long)blockIdx.x * ADJ_BLOCK + threadIdx.x;
    if (t >= live_cases(p)) return;
    const long long j = p.case_index ? p.case_index[t] : t;
    const int K = (int)p.max_nk;
    const int nk = max(min(p.nk[j * p.snk], K), 0);                   // never past the end of a row
    const bool uniform = (p.wm[j * p.swm] == WLSQM_WEIGHT_UNIFORM);
    unsigned long long known, dropped;
    effective_mask<NO>(p.knowns[j * p.sknowns], known, dropped);
    double xi[DIM];
    GeoLaneRows<DIM> rows;
    double* out = q.gxk + j * q.sgxk_j;
    double* gfk = q.gfk ? q.gfk + j * q.sgfk_j : nullptr;
    if (p.hoods) {
        const long long pj = own_point(p, j);
#pragma unroll
        for (int m = 0; m < DIM; ++m) xi[m] = p.S[pj * DIM + m];
        rows = GeoLaneRows<DIM>{nullptr, 0, p.hoods + j * p.shoods_j, p.S, nullptr, 0, p.F, out, q.sgxk_k, gfk, q.sgfk_k};
    } else {
#pragma unroll
        for (int m = 0; m < DIM; ++m) xi[m] = p.xi[j * p.sxi_j + m];
        rows = GeoLaneRows<DIM>{p.xk + j * p.sxk_j, p.sxk_k, nullptr, nullptr, p.fk + j * p.sfk_j, p.sfk_k, nullptr, out, q.sgxk_k,
                                gfk, q.sgfk_k};
    }
    geometry_adjoint_case<DIM, ORDER>(rows, xi, nk, K, uniform, known, dropped, q.g + j * q.sg_j, p.fi + j * p.sfi_j, q.gxi + j * q.sgxi_j);
}

// fk_image: the row of the image carries the case's K values of fk behind its K * DIM coordinates (dense rows of fk, and of grad_fk when
// it is wanted, and room within the LDS budget: geometry_fk_image); grad_fk[k] then overwrites fk[k] and leaves as the wave's contiguous
// run.  Otherwise each lane reads fk from, and writes grad_fk to, its own row in global memory.
template <int DIM, int ORDER>
__global__ __launch_bounds__(ADJ_BLOCK) void geometry_adjoint_rows_kernel(const KParams p, const GeometryAdjointArgs q, int pitch, int fk_image) {
    constexpr int NO = ndofs(DIM, ORDER);
    extern __shared__ double adj_lds[];
    const long long j0 = (long long)blockIdx.x * ADJ_BLOCK;
    const int K = (int)p.max_nk;
    const long long left = p.ncases - j0;
    const int ncw = left < ADJ_BLOCK ? (int)left : ADJ_BLOCK;          // the tail group has fewer than 64 cases
    adjoint_copy_run<true>(adj_lds, pitch, 1, const_cast<double*>(p.xk) + j0 * K * DIM, ncw, K * DIM);
    if (fk_image) adjoint_copy_run<true>(adj_lds + K * DIM, pitch, 1, const_cast<double*>(p.fk) + j0 * K, ncw, K);
    __syncthreads();
    if ((int)threadIdx.x < ncw) {
        const long long j = j0 + threadIdx.x;
        const int nk = max(min(p.nk[j * p.snk], K), 0);
        const bool uniform = (p.wm[j * p.swm] == WLSQM_WEIGHT_UNIFORM);
        unsigned long long known, dropped;
        effective_mask<NO>(p.knowns[j * p.sknowns], known, dropped);
        double xi[DIM];
#pragma unroll
        for (int m = 0; m < DIM; ++m) xi[m] = p.xi[j * p.sxi_j + m];
        double* row = adj_lds + (int)threadIdx.x * pitch;
        const GeoLdsRows<DIM> rows = fk_image
            ? GeoLdsRows<DIM>{row, row + K * DIM, 1, q.gfk ? row + K * DIM : nullptr, 1}
            : GeoLdsRows<DIM>{row, p.fk + j * p.sfk_j, p.sfk_k, q.gfk ? q.gfk + j * q.sgfk_j : nullptr, q.sgfk_k};
        geometry_adjoint_case<DIM, ORDER>(rows, xi, nk, K, uniform, known, dropped, q.g + j * q.sg_j, p.fi + j * p.sfi_j,
                                          q.gxi + j * q.sgxi_j);
    }
    __syncthreads();
    adjoint_copy_run<false>(adj_lds, pitch, 1, q.gxk + j0 * K * DIM, ncw, K * DIM);
    if (fk_image && q.gfk) adjoint_copy_run<false>(adj_lds + K * DIM, pitch, 1, q.gfk + j0 * K, ncw, K);
}

// The rows form's eligibility is the adjoint's (adjoint_rows_eligible), with grad_xk in xk's layout where the adjoint has grad_fk in fk's:
// dense rows of xk and of grad_xk, both bases 16-byte aligned, every case of the batch in order, the image within the LDS budget.
static bool geometry_rows_eligible(int dim, const KParams& p, const GeometryAdjointArgs& q, long long K) {
    if (p.hoods || p.case_index || p.ncases_dev || !p.xk || K < 1) return false;
    if (p.sxk_k != dim || p.sxk_j != K * dim || q.sgxk_k != dim || q.sgxk_j != K * dim) return false;
    if ((reinterpret_cast<uintptr_t>(p.xk) | reinterpret_cast<uintptr_t>(q.gxk)) & 15u) return false;
    return (size_t)adjoint_pitch(K * dim) * ADJ_BLOCK * sizeof(double) <= ADJ_LDS_BUDGET;
}

// Whether the rows form's image carries fk (and returns grad_fk) too: dense rows of fk, and of grad_fk when it is wanted, bases 16-byte
// aligned, and a row of K * (dim + 1) doubles still within the LDS budget (2D order 2 at 32 neighbours and 1D: yes; 3D order 2 at 40 and 2D
// order 4 at 64: no, 82 and 99 KiB).
static bool geometry_fk_image(int dim, const KParams& p, const GeometryAdjointArgs& q, long long K) {
    if (p.sfk_k != 1 || p.sfk_j != K || (reinterpret_cast<uintptr_t>(p.fk) & 15u)) return false;
    if (q.gfk && (q.sgfk_k != 1 || q.sgfk_j != K || (reinterpret_cast<uintptr_t>(q.gfk) & 15u))) return false;
    return (size_t)adjoint_pitch(K * (dim + 1)) * ADJ_BLOCK * sizeof(double) <= ADJ_LDS_BUDGET;
}

template <int DIM, int ORDER>
static int launch_geometry(const KParams& p, const GeometryAdjointArgs& q, bool rows, hipStream_t stream) {
    const long long blocks = (p.ncases + ADJ_BLOCK - 1) / ADJ_BLOCK;
    if (blocks <= 0) return WLSQM_OK;
    if (blocks > 0x7fffffffLL) { set_error("too many cases for one launch"); return WLSQM_EVALUE; }
    if (rows) {
        const int fk_image = geometry_fk_image(DIM, p, q, p.max_nk) ? 1 : 0;
        const int pitch = adjoint_pitch(p.max_nk * (DIM + fk_image));
        const size_t lds = (size_t)pitch * ADJ_BLOCK * sizeof(double);
        if (lds > 64 * 1024) {                                       // the opt-in to more than 64 KiB of dynamic LDS, once per device
            static bool opted[16] = {};
            int dev = 0;
            WLSQM_HIP_CHECK(hipGetDevice(&dev));
            if (dev < 0 || dev >= 16) { set_error("device ordinal out of range"); return WLSQM_EVALUE; }
            if (!opted[dev]) {
                WLSQM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&geometry_adjoint_rows_kernel<DIM, ORDER>),
                                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)ADJ_LDS_BUDGET));
                opted[dev] = true;
            }
        }
        hipLaunchKernelGGL((geometry_adjoint_rows_kernel<DIM, ORDER>), dim3((unsigned)blocks), dim3(ADJ_BLOCK), lds, stream, p, q, pitch,
                           fk_image);
        WLSQM_HIP_CHECK(hipGetLastError());
        note_kernel("geometry-adjoint-rows");
        return WLSQM_OK;
    }
    hipLaunchKernelGGL((geometry_adjoint_lane_kernel<DIM, ORDER>), dim3((unsigned)blocks), dim3(ADJ_BLOCK), 0, stream, p, q);
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("geometry-adjoint-lane");
    return WLSQM_OK;
}

int launch_fit_geometry_adjoint(int dimension, int order, const KParams& p, const GeometryAdjointArgs& q, hipStream_t stream) {
    if (p.ncases <= 0) return WLSQM_OK;
    const char form = env_first("WLSQM_HIP_ADJOINT_FORM");          // the adjoint's switch: =l the lane form, =r the rows form wherever eligible
    // unset: the rows form wherever it is eligible too; it measured faster at every shape of profiles/geometry_adjoint_timings.json
    const bool rows = form != 'l' && geometry_rows_eligible(dimension, p, q, p.max_nk);
#define CASE(D, O) if (dimension == D && order == O) return launch_geometry<D, O>(p, q, rows, stream);
    CASE(1, 0) CASE(1, 1) CASE(1, 2) CASE(1, 3) CASE(1, 4)
    CASE(2, 0) CASE(2, 1) CASE(2, 2) CASE(2, 3) CASE(2, 4)
    CASE(3, 0) CASE(3, 1) CASE(3, 2)
#undef CASE
    set_error("fit_geometry_adjoint: unsupported (dimension, order)");
    return WLSQM_EVALUE;
}

// ---- the stencil build: the adjoint's coefficients of a block of operators, stored as SELL-64 ------------------
// What StencilOperator's constructor assembles from one adjoint-lane launch per operator, a scatter and a pack, in one launch: one lane per
// case, which is one lane per row of the matrix, one wave per slice, so coefficient k of the 64 rows of a slice leaves as one contiguous
// 512-byte run per value plane.  Passes one and two are adjoint_case's (M, the knowns masked, ONE factorisation); then, for NB operators
// at a time, y_o = M_UU^-1 lambda_o and one pass over the neighbours that forms c_k and w_k once and stores w_k (c_k . y_o) for every
// operator of the block.  The statements of adjoint_case in its order: for the systems up to 10 unknowns (pin_fma) the coefficients are
// the bits of "adjoint-lane".  More than NB operators loop over the blocks with the factor in registers.
struct StencilBuildArgs {
    const double* lam; long long slam_o, slam_j;    // lambda[o, j, :] (slam_j == 0: the same operators at every case)
    int nop;
    const int32_t* len; const long long* soff;      // the frame: entry e of row j sits at soff[j / 64] + 64 e + j % 64 and is written iff e < len[j]
    int32_t* col;                                   // nullable: not written
    double* val; long long sval_o;
    double* kc; long long skc_o, skc_j;             // known_coef, nullable
};

// eliminate_knowns on the right-hand side with the knowns' values zero: g[a] = fma(-M[a, om], 0, g[a]) per known om.  It leaves a finite
// non-zero g[a] as it is; what it does to a zero (the sign) or when M[a, om] is not finite (NaN) it does to -0.0 as well, and adding
// that result to g[a] gives, bit for bit, what the chain started from g[a] gives.  So the chain runs once per case, on z = -0.0 (which
// masks M on the way, as pass two needs), and every operator's right-hand side is lambda + z (0 at the knowns).  z[a] is -0.0, +0.0
// or NaN: two bits per DOF (zpos, znan) carry it through the blocks.
template <int NO>
__device__ __forceinline__ void build_rhs(const double* lam, unsigned zpos, unsigned znan, unsigned long long known, double (&y)[NO]) {
#pragma unroll
    for (int a = 0; a < NO; ++a) {
        const double z = ((znan >> a) & 1u) ? __builtin_nan("") : ((zpos >> a) & 1u) ? 0.0 : -0.0;
        y[a] = ((known >> a) & 1ull) ? 0.0 : lam[a] + z;
    }
}

// Where the entries of row j go (entry e at at + 64 e) and how many of them may be written: e < len[j], and e < the slice's width, so
// that whatever nk, the mask and len say no write leaves the slice.
__device__ __forceinline__ void build_frame(const StencilBuildArgs& q, long long j, long long& at, int& live) {
    const long long s0 = q.soff[blockIdx.x];
    const long long wid = (q.soff[blockIdx.x + 1] - s0) >> 6;
    live = q.len[j];
    live = live < wid ? live : (int)wid;
    at = s0 + threadIdx.x;
}

// ONE: the launch has one operator (NB == 1), there is no loop over blocks and the factor dies with its only solve.  Beyond 10 unknowns
// the factor's 240 registers cannot stay live through pass three of a loop over blocks without scratch (profiles/isa_r06.txt): there, and
// there only, each lane parks its factor in LDS behind the factorisation (slot e of lane l at e * 64 + l: no bank conflicts, no barrier,
// a lane reads what it wrote) and every block's solve reads it back.
// At most two waves per SIMD: a lane walks its own row of hoods, so a wave's loads of hr[k] touch 64 lines that serve the next 32 values
// of k only while they stay in the CU's 32 KiB of L1.  Measured on 1M points of 2D order 2 at 24 neighbours: the one-operator kernel, whose 91
// registers would admit five waves, took 1.25 ms, the four-operator kernel (206 registers, two waves) 0.53 ms for three operators.
template <int DIM, int ORDER, int NB, bool ONE>
__global__ __launch_bounds__(ADJ_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 2))) void stencil_build_kernel(const KParams p, const StencilBuildArgs q) {
    constexpr int NO = ndofs(DIM, ORDER);
    constexpr int NE = NO * (NO + 1) / 2;
    constexpr bool PARK = !ONE && !pin_fma(NO);
    static_assert(!ONE || NB == 1, "one operator is a block of one");
    constexpr unsigned long long FULL = (1ull << NO) - 1ull;
    const long long j = (long long)blockIdx.x * ADJ_BLOCK + threadIdx.x;       // the row; blockIdx.x is the slice
    if (j >= p.ncases) return;
    const int K = (int)p.max_nk;
    const int nk = max(min(p.nk[j * p.snk], K), 0);                   // never past the end of a row
    const bool uniform = (p.wm[j * p.swm] == WLSQM_WEIGHT_UNIFORM);
    const long long raw = p.knowns[j * p.sknowns];
    unsigned long long known, dropped;
    effective_mask<NO>(raw, known, dropped);
    const bool fknown = (raw & 1ll) != 0;                            // the row ends in the entry of the point's own value
    const long long pj = own_point(p, j);
    const int* hr = p.hoods + j * p.shoods_j;
    if (known == FULL) {                            // nothing to solve: zeros on the neighbours, lambda in the known terms
        long long at; int live;
        build_frame(q, j, at, live);
        if (q.col) {
            for (int k = 0; k < nk; ++k)
                if (k < live) q.col[at + 64LL * k] = hr[k];
            if (fknown && nk < live) q.col[at + 64LL * nk] = (int32_t)pj;
        }
        for (int o = 0; o < q.nop; ++o) {
            const double* lo = q.lam + j * q.slam_j + o * q.slam_o;
            double* v = q.val + o * q.sval_o + at;
            for (int k = 0; k < nk; ++k)
                if (k < live) v[64LL * k] = 0.0;
            if (fknown && nk < live) v[64LL * nk] = lo[0];
            if (q.kc) {
                double* kc = q.kc + o * q.skc_o + j * q.skc_j;
#pragma unroll
                for (int a = 0; a < NO; ++a) kc[a] = (a == 0 && fknown) ? 0.0 : lo[a];
            }
        }
        return;
    }
    double xi[DIM];
#pragma unroll
    for (int m = 0; m < DIM; ++m) xi[m] = p.S[pj * DIM + m];
    const AdjLaneRows<DIM> rows{nullptr, 0, hr, p.S, nullptr, 0};
    // pass 1: largest squared distance; not needed for uniform weights
    double max_d2 = 0.0;
    if (!uniform) {
        for (int k = 0; k < nk; ++k) {
            double d[DIM];
            rows.offset(k, xi, d);
            double d2 = d[0] * d[0];
            if constexpr (DIM >= 2) d2 += d[1] * d[1];
            if constexpr (DIM == 3) d2 += d[2] * d[2];
            if (d2 > max_d2) max_d2 = d2;
        }
    }
    const double inv_max = inverse_max(max_d2);
    // pass 2: M = C^T W C (upper triangle)
    double M[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) M[e] = 0.0;
    for (int k = 0; k < nk; ++k) {
        double d[DIM], c[NO];
        rows.offset(k, xi, d);
        const double d2 = monomials<DIM, ORDER>(d, c);
        accumulate_matrix<NO>(M, c, weight(d2, inv_max, uniform));
    }
    // knowns: rows and columns masked to identity; z is what the elimination does to a right-hand side (build_rhs)
    unsigned zpos = 0, znan = 0;
    {
        double zero[NO], z[NO];
#pragma unroll
        for (int a = 0; a < NO; ++a) { zero[a] = 0.0; z[a] = -0.0; }
        eliminate_knowns<NO>(M, z, known, zero);
#pragma unroll
        for (int a = 0; a < NO; ++a) {
            if (z[a] != z[a]) znan |= 1u << a;
            else if (!__builtin_signbit(z[a])) zpos |= 1u << a;
        }
    }
    ldlt_factor<NO>(M);
    __shared__ double parked[PARK ? NE * ADJ_BLOCK : 1];
    if constexpr (PARK) {
#pragma unroll
        for (int e = 0; e < NE; ++e) parked[e * ADJ_BLOCK + threadIdx.x] = M[e];
    }
    const bool sums = (known & ~dropped) != 0ull;
    // the frame and the operators' addresses are formed here, behind the factorisation, which has no register to spare for them
    long long at; int live;
    build_frame(q, j, at, live);
    const double* lam = q.lam + j * q.slam_j;
    const int nop = ONE ? 1 : q.nop;
    for (int o0 = 0; o0 < nop; o0 += NB) {
        const int nb = nop - o0 < NB ? nop - o0 : NB;                // wave-uniform
        double y[NB][NO], acc[NB][NO];
        if constexpr (PARK) {
            __asm__ volatile("" ::: "memory");      // the loads stay inside the loop: hoisted, the factor would be live through pass three again
#pragma unroll
            for (int e = 0; e < NE; ++e) M[e] = parked[e * ADJ_BLOCK + threadIdx.x];
        }
#pragma unroll
        for (int o = 0; o < NB; ++o) {
            build_rhs<NO>(lam + (o0 + (o < nb ? o : 0)) * q.slam_o, zpos, znan, known, y[o]);
            ldlt_solve<NO>(M, y[o]);                // y_U = M_UU^-1 lambda_U, y = 0 outside U
#pragma unroll
            for (int a = 0; a < NO; ++a) acc[o][a] = 0.0;
        }
        // pass 3: w_k (c_k . y_o) into the value planes; the true knowns' columns collect sum_k c_k[a] (.) = (M y_o)[a]
        double* val = q.val + o0 * q.sval_o + at;
#pragma unroll 1
        for (int k = 0; k < nk; ++k) {
            double d[DIM], c[NO];
            rows.offset(k, xi, d);
            const double d2 = monomials<DIM, ORDER>(d, c);
            const double w = weight(d2, inv_max, uniform);
            if (o0 == 0 && q.col && k < live) q.col[at + 64LL * k] = hr[k];
#pragma unroll
            for (int o = 0; o < NB; ++o) {
                double s = y[o][0];
#pragma unroll
                for (int a = 1; a < NO; ++a) s = fma(c[a], y[o][a], s);
                const double gk = w * s;
                if (o < nb && k < live) val[o * q.sval_o + 64LL * k] = gk;
                if (sums) {
                    // adjoint_case's `acc[0] += gk` leaves the compiler the choice to contract gk = w * s into the sum, and it chooses by
                    // the size of the loop: "adjoint-lane" has fma(w, s, acc[0]) up to 3 unknowns (the loop is unswitched on `sums`, product
                    // and sum share a block) and the plain sum from 4 on (read from its ISA, all 13 instantiations; tests/
                    // test_gpu_stencil_update.py holds every system up to 10 unknowns to the constructor's bits).  Spelled out either way.
                    if constexpr (NO <= 3) {
                        acc[o][0] = fma(w, s, acc[o][0]);
                    } else {
#pragma clang fp contract(off)
                        acc[o][0] = acc[o][0] + gk;
                    }
#pragma unroll
                    for (int a = 1; a < NO; ++a) acc[o][a] = fma(c[a], gk, acc[o][a]);
                }
            }
        }
        if (o0 == 0 && q.col && fknown && nk < live) q.col[at + 64LL * nk] = (int32_t)pj;
#pragma unroll
        for (int o = 0; o < NB; ++o) {
            if (o < nb) {
                const double* gb = lam + (o0 + o) * q.slam_o;         // read again: a copy of lambda beside the factor costs the 15-unknown system scratch
                if (fknown && nk < live) val[o * q.sval_o + 64LL * nk] = gb[0] - acc[o][0];
                if (q.kc) {
                    double* kc = q.kc + (o0 + o) * q.skc_o + j * q.skc_j;
#pragma unroll
                    for (int a = 0; a < NO; ++a) {
                        double v = 0.0;                                          // an unknown's incoming value is never read by the fit
                        if ((known >> a) & 1ull) v = ((dropped >> a) & 1ull) ? gb[a] : gb[a] - acc[o][a];
                        kc[a] = (a == 0 && fknown) ? 0.0 : v;
                    }
                }
            }
        }
    }
}

// Operators per block: what the register file carries beside the factor without scratch (profiles/isa_r06.txt).
constexpr int stencil_build_block(int no) { return no <= 6 ? 4 : no <= 10 ? 2 : 1; }

template <int DIM, int ORDER>
static int launch_stencil_build(const KParams& p, const StencilBuildArgs& q, hipStream_t stream) {
    constexpr int NB = stencil_build_block(ndofs(DIM, ORDER));
    const long long blocks = (p.ncases + ADJ_BLOCK - 1) / ADJ_BLOCK;
    if (blocks > 0x7fffffffLL) { set_error("too many cases for one launch"); return WLSQM_EVALUE; }
    if (q.nop == 1) hipLaunchKernelGGL((stencil_build_kernel<DIM, ORDER, 1, true>), dim3((unsigned)blocks), dim3(ADJ_BLOCK), 0, stream, p, q);
    else hipLaunchKernelGGL((stencil_build_kernel<DIM, ORDER, NB, false>), dim3((unsigned)blocks), dim3(ADJ_BLOCK), 0, stream, p, q);
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("stencil-build");
    return WLSQM_OK;
}

static int launch_stencil_build_any(int dimension, int order, const KParams& p, const StencilBuildArgs& q, hipStream_t stream) {
#define CASE(D, O) if (dimension == D && order == O) return launch_stencil_build<D, O>(p, q, stream);
    CASE(1, 0) CASE(1, 1) CASE(1, 2) CASE(1, 3) CASE(1, 4)
    CASE(2, 0) CASE(2, 1) CASE(2, 2) CASE(2, 3) CASE(2, 4)
    CASE(3, 0) CASE(3, 1) CASE(3, 2)
#undef CASE
    set_error("fit_adjoint: unsupported (dimension, order)");
    return WLSQM_EVALUE;
}

}  // namespace wlsqm

using namespace wlsqm;

extern "C" {

int wlsqm_hip_stencil_build_device(int dimension, int order, int64_t ncases, int64_t max_nk,
                                   const double* S, const int32_t* hoods, int64_t hoods_stride_case,
                                   const int32_t* point_index, const int32_t* nk, const int64_t* knowns,
                                   const int32_t* weighting_method,
                                   const double* rows, int64_t rows_stride_op, int64_t rows_stride_case, int nop,
                                   const int32_t* len, const int64_t* soff, int32_t* col, double* val, int64_t val_stride_op,
                                   double* known_coef, int64_t kc_stride_op, int64_t kc_stride_case, int device, void* stream) {
    if (dimension < 1 || dimension > 3) { set_error("dimension must be 1, 2 or 3"); return WLSQM_EVALUE; }
    const int no = wlsqm_hip_number_of_dofs(dimension, order);
    if (no < 0) { set_error("order must be 0..4"); return WLSQM_EVALUE; }
    if (ncases < 0) { set_error("ncases must be >= 0"); return WLSQM_EVALUE; }
    if (max_nk < 0) { set_error("max_nk must be >= 0"); return WLSQM_EVALUE; }
    if (nop < 1) { set_error("stencil_build: nop must be >= 1"); return WLSQM_EVALUE; }
    if (ncases > 0 && (!S || !hoods || !nk || !knowns || !weighting_method || !rows || !len || !soff || !val)) { set_error("null array"); return WLSQM_EVALUE; }
    if (known_coef && kc_stride_case < no) { set_error("gradient rows narrower than the number of DOFs"); return WLSQM_EVALUE; }
    if (hoods_stride_case < max_nk) { set_error("hoods rows narrower than max_nk"); return WLSQM_EVALUE; }
    DeviceScope scope;
    const int rc = scope.enter(device);
    if (rc != WLSQM_OK || ncases == 0) return rc;
    KParams p{};
    p.hoods = hoods; p.shoods_j = hoods_stride_case; p.S = S; p.pidx = point_index;
    p.nk = nk; p.snk = 1; p.knowns = (const long long*)knowns; p.sknowns = 1; p.wm = weighting_method; p.swm = 1;
    p.ncases = ncases; p.max_nk = max_nk;
    const StencilBuildArgs q{rows, rows_stride_op, rows_stride_case, nop, len, reinterpret_cast<const long long*>(soff), col, val, val_stride_op,
                             known_coef, kc_stride_op, kc_stride_case};
    return launch_stencil_build_any(dimension, order, p, q, (hipStream_t)stream);
}

}  // extern "C"
