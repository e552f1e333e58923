// interp_plan.hip — device-resident interpolation plans: "these models evaluated at these points", searched once, evaluated many times.
//
// ExpertSolver.interpolate (expert.pyx:687-985) searches the origins and evaluates one `diff` per call, from host arrays (expert.hip,
// interp.hip, knn.hip).  The origins are fixed after prepare() and the evaluation points usually are too, so a plan keeps what does not
// depend on the coefficients — packed copies of the origins xi[nmodels, dim], the orders and the points x[nx, dim], and per point either
// the model number (mode 0, nearest: nearest_search of knn.hip, or the caller's I) or the CSR list of the models within r (mode 1,
// continuous: two grid walks, count and fill, around an exclusive scan) — and its evaluate call only enqueues ONE kernel on the caller's
// stream: no allocation, no copy, no synchronisation, so it can be captured into a graph behind the solve that makes the coefficients.
//
// List order (continuous): the cells of the uniform grid over the origins that the ball's bounding block touches, rows of cells in
// ascending (z, y), the cells of a row in ascending x, the origins of a cell in ascending model number (the grid's sort is stable).
// It is a function of the inputs alone: two plans of the same inputs hold the same lists.  Model numbers are stored as int32.
//
// The evaluation kernel computes EVERY derivative of the model at once: with c[b] = prod_m (x_m - xi_m)^(P_b)_m / (P_b)_m! the scaled
// monomials of the offset (built once per point and model) and P the exponent table of the DOFs (defs.pyx:91-183),
//     d^Q model (x) = sum_{a : P_a >= Q} fi[a] * c[index of P_a - Q],
// so the pair (a, b) with P_b <= P_a feeds the derivative number index(P_a - P_b): all three indices are compile-time constants of a
// fully unrolled double loop (C(2 dim + order, order) fused multiply-adds: 15 for 2D order 2, 210 for 3D order 4), every coefficient is
// read once, and the requested diffs are picked from the registers at the store.  Because every derivative is accumulated by the same
// instruction sequence whatever was asked for, a value does not depend on its companions in the call: diff d alone, among others, in
// any position or repeated, its field alone or in a stack, eager or replayed — the same bits.  The rounding sequence is in the source:
// the translation unit compiles without contraction and every fused operation is a spelled-out fma.
#include <algorithm>
#include <new>
#include <utility>

#include <hipcub/hipcub.hpp>

#include "wlsqm_dispatch.hpp"
#include "wlsqm_grid.hpp"
#include "wlsqm_interp.hpp"

#pragma clang fp contract(off)      // a * b + c below is two roundings; the fused sums are __builtin_fma

namespace wlsqm {

template <class F, int... Is>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, Is...>) {
    (f(std::integral_constant<int, Is>{}), ...);
}
// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a loop whose counter is a constant expression in the body
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }

// DOF number of the monomial x^p y^q z^r (-1: none up to order 4)
template <int DIM>
__host__ __device__ constexpr int mono_index(int p, int q, int r) {
    for (int a = 0; a < ndofs(DIM, 4); ++a)
        if (Mono<DIM>::P[a] == p && Mono<DIM>::Q[a] == q && Mono<DIM>::R[a] == r) return a;
    return -1;
}
template <int DIM>
__host__ __device__ constexpr int mono_degree(int a) { return Mono<DIM>::P[a] + Mono<DIM>::Q[a] + Mono<DIM>::R[a]; }

struct PlanDiffs { int n; int d[35]; };     // the requested diffs, by value (-1: a diff no model of the plan has, gives 0)

struct PlanEval {
    const double* xi; const int* order; long long nmodels;      // packed origins [nmodels, dim] and orders
    const double* x; long long nx;                              // packed points [nx, dim]
    const long long* I;                                         // nearest: model of point m
    const long long* off; const int* idx; double r2;            // continuous: CSR lists
    const double* fi; long long sfi_f, sfi_m; long long nfields;
    double* out; long long so_f, so_d;
};

// offset d of xp from the origin xo and its squared length; the list builder computes d2 by the same expression on the same numbers,
// so every member of a list has d2 <= r2 here as well.  The squares are rounded before they are added, (d0^2 + d1^2) + d2^2, which is
// the sequence interp_kernel (interp.hip over eval_model) compiles to: near the sphere 1 - sqrt(d2 / r2) cancels, one ulp of d2 is a
// relative eps / t of the weight, and a fused sum here would move the weighted average away from the list-taking entry point's by
// more than the arithmetic of the models does.  With this sequence the weights of the two routes are the same bits.
template <int DIM>
__device__ __forceinline__ double offset_of(const double (&xp)[DIM], const double* __restrict__ xo, double (&d)[DIM]) {
    double d2 = 0.0;
#pragma unroll
    for (int m = 0; m < DIM; ++m) {
        d[m] = xp[m] - xo[m];
        const double sq = __dmul_rn(d[m], d[m]);
        d2 = m == 0 ? sq : __dadd_rn(d2, sq);
    }
    return d2;
}

template <int DIM, int MAXORD>
__device__ __forceinline__ void monomial_table(const double (&d)[DIM], double (&c)[ndofs(DIM, MAXORD)]) {
    double pw[DIM][5];
#pragma unroll
    for (int m = 0; m < DIM; ++m) {
        const double dd = d[m] * d[m];
        pw[m][0] = 1.0; pw[m][1] = d[m]; pw[m][2] = 0.5 * dd; pw[m][3] = ((1.0 / 6.0) * dd) * d[m]; pw[m][4] = ((1.0 / 24.0) * dd) * dd;
    }
    static_for<ndofs(DIM, MAXORD)>([&](auto bc) {
        constexpr int b = decltype(bc)::value;
        double v = pw[0][Mono<DIM>::P[b]];
        if constexpr (DIM >= 2) v = v * pw[1][Mono<DIM>::Q[b]];
        if constexpr (DIM == 3) v = v * pw[2][Mono<DIM>::R[b]];
        c[b] = v;
    });
}

// v[Q] = d^Q model for every DOF number Q < ndofs(DIM, MAXORD): 0 where Q >= the model's own no.  Terms enter v[Q] in ascending a.
template <int DIM, int MAXORD>
__device__ __forceinline__ void eval_all(const double* __restrict__ f, int order, const double (&c)[ndofs(DIM, MAXORD)],
                                         double (&v)[ndofs(DIM, MAXORD)]) {
    constexpr int NO = ndofs(DIM, MAXORD);
    static_for<NO>([&](auto ic) { v[decltype(ic)::value] = 0.0; });
    static_for<MAXORD + 1>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        if (order >= k) {                                       // the DOFs of degree k exist in this model: only those are read
            static_for<NO>([&](auto ac) {
                constexpr int a = decltype(ac)::value;
                if constexpr (mono_degree<DIM>(a) == k) {
                    const double fa = f[a];
                    static_for<a + 1>([&](auto bc) {
                        constexpr int b = decltype(bc)::value;
                        constexpr int p = Mono<DIM>::P[a] - Mono<DIM>::P[b], q = Mono<DIM>::Q[a] - Mono<DIM>::Q[b],
                                      r = Mono<DIM>::R[a] - Mono<DIM>::R[b];
                        if constexpr (p >= 0 && q >= 0 && r >= 0) {
                            constexpr int Q = mono_index<DIM>(p, q, r);
                            v[Q] = __builtin_fma(fa, c[b], v[Q]);
                        }
                    });
                }
            });
        }
    });
}

// out[f][j][m] = v[D.d[j]] (`none` for D.d[j] < 0); the diffs are wave-uniform, so this is scalar control flow around ndiff stores
template <int NO>
__device__ __forceinline__ void store_diffs(const PlanEval& q, const PlanDiffs& D, long long f, long long m, const double (&v)[NO],
                                            double none) {
    double* __restrict__ o = q.out + f * q.so_f + m;
    static_for<NO>([&](auto ic) {
        constexpr int Q = decltype(ic)::value;
        for (int j = 0; j < D.n; ++j)
            if (D.d[j] == Q) o[j * q.so_d] = v[Q];
    });
    for (int j = 0; j < D.n; ++j)
        if (D.d[j] < 0) o[j * q.so_d] = none;
}

// One lane per evaluation point.  Nearest: the table of the point's one model is built once and serves every field.  Continuous: the
// list is walked once per field (offset, weight and table are recomputed per field: a stack costs nfields walks, one field costs one).
template <int DIM, int MAXORD, bool CONT>
__global__ __launch_bounds__(256) void interp_plan_eval_kernel(const PlanEval q, const PlanDiffs D) {
    constexpr int NO = ndofs(DIM, MAXORD);
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= q.nx) return;
    double xp[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) xp[c] = q.x[m * DIM + c];
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double c[NO], v[NO], d[DIM];
    if constexpr (!CONT) {
        const long long model = q.I[m];
        if (model < 0 || model >= q.nmodels) {
            for (long long f = 0; f < q.nfields; ++f)
                for (int j = 0; j < D.n; ++j) q.out[f * q.so_f + j * q.so_d + m] = nan;
            return;
        }
        const int order = q.order[model];
        (void)offset_of<DIM>(xp, q.xi + model * DIM, d);
        monomial_table<DIM, MAXORD>(d, c);
        for (long long f = 0; f < q.nfields; ++f) {
            eval_all<DIM, MAXORD>(q.fi + f * q.sfi_f + model * q.sfi_m, order, c, v);
            store_diffs<NO>(q, D, f, m, v, 0.0);
        }
    } else {
        const long long e0 = q.off[m], e1 = q.off[m + 1];
        for (long long f = 0; f < q.nfields; ++f) {
            double acc[NO], sum_w = 0.0;
            static_for<NO>([&](auto ic) { acc[decltype(ic)::value] = 0.0; });
            for (long long e = e0; e < e1; ++e) {
                const long long model = q.idx[e];
                const double d2 = offset_of<DIM>(xp, q.xi + model * DIM, d);
                monomial_table<DIM, MAXORD>(d, c);
                eval_all<DIM, MAXORD>(q.fi + f * q.sfi_f + model * q.sfi_m, q.order[model], c, v);
                const double t = 1.0 - sqrt(d2 / q.r2);         // expert.pyx:45-46: alpha = 0, beta = 1
                const double w = t * t;
                static_for<NO>([&](auto ic) { constexpr int Q = decltype(ic)::value; acc[Q] = __builtin_fma(w, v[Q], acc[Q]); });
                sum_w = sum_w + w;
            }
            static_for<NO>([&](auto ic) { constexpr int Q = decltype(ic)::value; v[Q] = acc[Q] / sum_w; });   // empty list: 0/0 = NaN
            store_diffs<NO>(q, D, f, m, v, 0.0 / sum_w);       // a diff no model has: 0, NaN on an empty list
        }
    }
}

// The grid walk of interp_ball_kernel (knn.hip), twice: FILL = false counts the origins within r of every point, FILL = true writes
// their numbers at the point's offset.  Both passes test the same d2 <= r2 on the same numbers, so the counts are the lists' lengths.
template <int DIM, bool FILL>
__global__ __launch_bounds__(64) void interp_plan_ball_kernel(const double* __restrict__ Ss, const int* __restrict__ perm,
                                                              const int* __restrict__ start, KnnGrid G, const double* __restrict__ x,
                                                              long long nx, double r, long long* __restrict__ cnt,
                                                              const long long* __restrict__ off, int* __restrict__ idx) {
    const long long m = (long long)blockIdx.x * 64 + threadIdx.x;
    if (m >= nx) return;
    double xp[DIM], d[DIM]; int c0[3] = {0, 0, 0}, c1[3] = {0, 0, 0};
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
        xp[c] = x[m * DIM + c];
        c0[c] = cell_coord(xp[c] - r, G, c); c1[c] = cell_coord(xp[c] + r, G, c);
    }
    const double r2 = r * r;
    long long n = 0, e = FILL ? off[m] : 0;
    for (int cz = c0[2]; cz <= c1[2]; ++cz)
        for (int cy = c0[1]; cy <= c1[1]; ++cy) {
            const long long row = (long long)G.g[0] * (cy + (long long)G.g[1] * cz);
            const int p0 = start[row + c0[0]], p1 = start[row + c1[0] + 1];
            for (int pos = p0; pos < p1; ++pos) {
                if (offset_of<DIM>(xp, Ss + (long long)pos * DIM, d) > r2) continue;
                if constexpr (FILL) idx[e++] = perm[pos]; else ++n;
            }
        }
    if constexpr (!FILL) cnt[m] = n;
}

__global__ void interp_plan_pack_rows_kernel(const double* __restrict__ src, long long stride, long long n, int dim,
                                             double* __restrict__ dst) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int c = 0; c < dim; ++c) dst[i * dim + c] = src[i * stride + c];
}

// flags[0] = 1 when some order is outside 0..4, flags[1] = the largest order
__global__ void interp_plan_pack_order_kernel(const int* __restrict__ src, long long stride, long long n, int* __restrict__ dst,
                                              int* __restrict__ flags) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int o = src[i * stride];
    dst[i] = o;
    if (o < 0 || o > 4) atomicMax(&flags[0], 1); else atomicMax(&flags[1], o);
}

__global__ void interp_plan_widen_kernel(const int* __restrict__ src, long long n, long long* __restrict__ dst) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// ---- the adjoint of the evaluation ----
// evaluate is linear in fi, and the search, the offsets and the weights do not depend on fi, so its adjoint is a scatter-add of
// g[f, j, m] times scaled monomials into the coefficient rows.  It is computed as a GATHER over the inverted index of the plan (per
// model the points that use it, in ascending point number: toff / tpt), so that every element of grad_fi has one writer and a fixed
// summation order: no atomics, the bits are a function of the plan and of the field's g.
//     nearest:     grad_fi[f, i, a] = sum_{m : I_m == i} sum_{j : P_a >= P_Qj} g[f, j, m] c_m[index(P_a - P_Qj)]
//     continuous:  the same over the list entries (m, e) with idx[e] == i, every term scaled by w_{m,e} / W_m
// Contributions are recomputed from x_m and g, never stored: a stored row would cost more bytes than the point and its g.

constexpr int kAdjointLong = 64;     // models with MORE entries than this take the wave form (one wave's worth: below it lanes would idle)

struct PlanAdj {
    const double* xi; const int* order; long long nmodels;
    const double* x;
    const long long* toff; const int* tpt;                       // inverted index: the entries of model i are tpt[toff[i] : toff[i + 1]]
    const double* W; double r2;                                  // continuous: W[m] = the forward's sum of weights of point m
    const int* longs; long long nlong;                           // the models with more than kAdjointLong entries, ascending
    const double* g; long long sg_f, sg_d; long long nfields;
    double* gfi; long long sgfi_f, sgfi_m; int ncols;
};

// acc[a] += scale * g[f, j, m] * c[index(P_a - P_Qj)] for one entry (point m of the model at xo) and every requested diff: the diffs in
// ascending DOF number Q, repeats in call order (they travel by value: scalar control flow, as in store_diffs), the a of a diff in
// ascending DOF number.  A diff the model does not have (degree above its order) and a point with W_m == 0 contribute nothing and their
// g is not read.
template <int DIM, int MAXORD, bool CONT>
__device__ __forceinline__ void adjoint_entry(const PlanAdj& q, const PlanDiffs& D, long long f, long long m, const double* xo, int order,
                                              double (&acc)[ndofs(DIM, MAXORD)]) {
    constexpr int NO = ndofs(DIM, MAXORD);
    double xp[DIM], d[DIM], c[NO];
#pragma unroll
    for (int k = 0; k < DIM; ++k) xp[k] = q.x[m * DIM + k];
    const double d2 = offset_of<DIM>(xp, xo, d);
    double scale = 1.0;
    if constexpr (CONT) {
        const double W = q.W[m];
        if (W == 0.0) return;                                    // the forward's value there is 0 / 0: it does not depend on fi
        const double t = 1.0 - sqrt(d2 / q.r2);                  // the forward's weight, by the forward's sequence
        const double w = t * t;
        scale = w / W;
    }
    monomial_table<DIM, MAXORD>(d, c);
    const double* __restrict__ gm = q.g + f * q.sg_f + m;
    static_for<NO>([&](auto qc) {
        constexpr int Q = decltype(qc)::value;
        constexpr int kq = mono_degree<DIM>(Q);
        if (order >= kq) {
            for (int j = 0; j < D.n; ++j) {
                if (D.d[j] != Q) continue;
                double gq = gm[j * q.sg_d];
                if constexpr (CONT) gq = scale * gq;
                static_for<MAXORD + 1 - kq>([&](auto kc) {
                    constexpr int k = kq + decltype(kc)::value;
                    if (order >= k) {
                        static_for<NO>([&](auto ac) {
                            constexpr int a = decltype(ac)::value;
                            constexpr int p = Mono<DIM>::P[a] - Mono<DIM>::P[Q], s = Mono<DIM>::Q[a] - Mono<DIM>::Q[Q],
                                          r = Mono<DIM>::R[a] - Mono<DIM>::R[Q];
                            if constexpr (mono_degree<DIM>(a) == k && p >= 0 && s >= 0 && r >= 0) {
                                constexpr int b = mono_index<DIM>(p, s, r);
                                acc[a] = __builtin_fma(gq, c[b], acc[a]);
                            }
                        });
                    }
                });
            }
        }
    });
}

// ncols columns of the row: the accumulators (zero from the model's own no on: nothing was added there), then zeros
template <int NO>
__device__ __forceinline__ void adjoint_store_row(const PlanAdj& q, long long f, long long i, const double (&acc)[NO]) {
    double* __restrict__ row = q.gfi + f * q.sgfi_f + i * q.sgfi_m;
    static_for<NO>([&](auto ac) { constexpr int a = decltype(ac)::value; if (a < q.ncols) row[a] = acc[a]; });
    for (int a = NO; a < q.ncols; ++a) row[a] = 0.0;
}

// Lane form: one lane per model walks its entries in ascending point number.  Long models are left to the wave form.
template <int DIM, int MAXORD, bool CONT>
__global__ __launch_bounds__(256) void interp_plan_adjoint_lane_kernel(const PlanAdj q, const PlanDiffs D) {
    constexpr int NO = ndofs(DIM, MAXORD);
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= q.nmodels) return;
    const long long t0 = q.toff[i], t1 = q.toff[i + 1];
    if (t1 - t0 > kAdjointLong) return;
    const int order = q.order[i];
    double xo[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) xo[k] = q.xi[i * DIM + k];
    for (long long f = 0; f < q.nfields; ++f) {
        double acc[NO];
        static_for<NO>([&](auto ac) { acc[decltype(ac)::value] = 0.0; });
        if (D.n > 0)
            for (long long e = t0; e < t1; ++e) adjoint_entry<DIM, MAXORD, CONT>(q, D, f, q.tpt[e], xo, order, acc);
        adjoint_store_row<NO>(q, f, i, acc);
    }
}

// Wave form: one wavefront per long model.  Lane l takes the entries l, l + 64, ... in that order into private accumulators, a fixed
// butterfly adds the 64 partial sums (every lane ends with the same bits: a + b == b + a), lane 0 stores the row.  The order of the sum
// depends on the length of the list alone.
template <int DIM, int MAXORD, bool CONT>
__global__ __launch_bounds__(256) void interp_plan_adjoint_wave_kernel(const PlanAdj q, const PlanDiffs D) {
    constexpr int NO = ndofs(DIM, MAXORD);
    const long long slot = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= q.nlong) return;
    const int lane = threadIdx.x & 63;
    const long long i = q.longs[slot];
    const long long t0 = q.toff[i], t1 = q.toff[i + 1];
    const int order = q.order[i];
    double xo[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) xo[k] = q.xi[i * DIM + k];
    for (long long f = 0; f < q.nfields; ++f) {
        double acc[NO];
        static_for<NO>([&](auto ac) { acc[decltype(ac)::value] = 0.0; });
        if (D.n > 0)
            for (long long e = t0 + lane; e < t1; e += 64) adjoint_entry<DIM, MAXORD, CONT>(q, D, f, q.tpt[e], xo, order, acc);
        static_for<NO>([&](auto ac) {
            constexpr int a = decltype(ac)::value;
            if (order >= mono_degree<DIM>(a)) {                  // wave-uniform: the other accumulators are zero in every lane
#pragma unroll
                for (int step = 32; step >= 1; step >>= 1) acc[a] = acc[a] + __shfl_xor(acc[a], step, 64);
            }
        });
        if (lane == 0) adjoint_store_row<NO>(q, f, i, acc);
    }
}

// W[m] = sum of the weights of point m's list by the forward's own sequence (offset_of, 1 - sqrt(d2 / r2), t * t, sum_w + w in list
// order): the forward's bits
template <int DIM>
__global__ __launch_bounds__(256) void interp_plan_weight_sum_kernel(const double* __restrict__ xi, const double* __restrict__ x,
                                                                     long long nx, const long long* __restrict__ off,
                                                                     const int* __restrict__ idx, double r2, double* __restrict__ W) {
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= nx) return;
    double xp[DIM], d[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) xp[c] = x[m * DIM + c];
    double sum_w = 0.0;
    for (long long e = off[m]; e < off[m + 1]; ++e) {
        const double d2 = offset_of<DIM>(xp, xi + (long long)idx[e] * DIM, d);
        const double t = 1.0 - sqrt(d2 / r2);
        const double w = t * t;
        sum_w = sum_w + w;
    }
    W[m] = sum_w;
}

// the (model, point) pairs to sort.  Nearest: one per point, an I outside 0 .. nmodels - 1 gets the key nmodels (sorts behind every
// model and is dropped).  Continuous: one per list entry.
__global__ void interp_plan_pairs_nearest_kernel(const long long* __restrict__ I, long long nx, long long nmodels,
                                                 unsigned* __restrict__ key, int* __restrict__ val) {
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= nx) return;
    const long long model = I[m];
    key[m] = (unsigned)((model < 0 || model >= nmodels) ? nmodels : model);
    val[m] = (int)m;
}

__global__ void interp_plan_pairs_lists_kernel(const long long* __restrict__ off, const int* __restrict__ idx, long long nx,
                                               unsigned* __restrict__ key, int* __restrict__ val) {
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= nx) return;
    for (long long e = off[m]; e < off[m + 1]; ++e) { key[e] = (unsigned)idx[e]; val[e] = (int)m; }
}

// toff[i] = the first position of the sorted keys that holds a key >= i (i = 0 .. nmodels: toff[nmodels] is the number of entries)
__global__ void interp_plan_offsets_kernel(const unsigned* __restrict__ key, long long n, long long nmodels, long long* __restrict__ toff) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nmodels) return;
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if ((long long)key[mid] < i) lo = mid + 1; else hi = mid;
    }
    toff[i] = lo;
}

// len[i] and flag[i] = 1 for a long model (i < nmodels); len[nmodels] = flag[nmodels] = 0 closes the scan
__global__ void interp_plan_lengths_kernel(const long long* __restrict__ toff, long long nmodels, long long* __restrict__ len,
                                           long long* __restrict__ flag) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nmodels) return;
    const long long n = i < nmodels ? toff[i + 1] - toff[i] : 0;
    len[i] = n;
    flag[i] = n > kAdjointLong ? 1 : 0;
}

__global__ void interp_plan_compact_long_kernel(const long long* __restrict__ len, const long long* __restrict__ pos, long long nmodels,
                                                int* __restrict__ longs) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nmodels && len[i] > kAdjointLong) longs[pos[i]] = (int)i;
}

}  // namespace wlsqm

using namespace wlsqm;

struct wlsqm_interp_plan {
    int device = 0, dimension = 0, mode = 0, max_order = 0;
    int64_t nmodels = 0, nx = 0, nlist = 0, max_list = 0;
    double r = 0.0;
    DevBuf d_xi, d_order, d_x, d_I, d_off, d_idx;
    // the inverted index of the adjoint (build_adjoint_index): absent until prepare_adjoint or the first adjoint call
    bool adj_ready = false;
    int64_t adj_entries = 0, adj_max_len = 0, adj_nlong = 0;
    DevBuf d_toff, d_tpt, d_W, d_long;
    int64_t bytes() const {
        return (int64_t)(d_xi.n + d_order.n + d_x.n + d_I.n + d_off.n + d_idx.n + d_toff.n + d_tpt.n + d_W.n + d_long.n);
    }
};

static inline unsigned blocks_of(long long n, int per) { return (unsigned)((n + per - 1) / per); }

// continuous mode: count, scan, fill
static int build_lists(wlsqm_interp_plan& P, hipStream_t s) {
    int rc;
    const int dim = P.dimension; const long long nx = P.nx;
    if ((rc = P.d_off.alloc((size_t)(nx + 1) * 8))) return rc;
    if (nx == 0) { WLSQM_HIP_CHECK(hipMemsetAsync(P.d_off.p, 0, 8, s)); return P.d_idx.alloc(4); }
    GridIndex grid;
    if ((rc = grid.build(dim, P.nmodels, P.d_xi.as<double>(), s))) return rc;
    DevBuf d_cnt, d_max, d_tmp;
    if ((rc = d_cnt.alloc((size_t)(nx + 1) * 8)) || (rc = d_max.alloc(8))) return rc;
    WLSQM_HIP_CHECK(hipMemsetAsync(d_cnt.p, 0, d_cnt.n, s));
    const unsigned blocks = blocks_of(nx, 64);
#define PLAN_BALL(D, FILL)                                                                                                       \
    hipLaunchKernelGGL((interp_plan_ball_kernel<D, FILL>), dim3(blocks), dim3(64), 0, s, grid.d_Ss.as<double>(), grid.d_perm.as<int>(), \
                       grid.d_start.as<int>(), grid.G, P.d_x.as<double>(), nx, P.r, d_cnt.as<long long>(),                   \
                       P.d_off.as<long long>(), P.d_idx.as<int>());
    if (dim == 1) PLAN_BALL(1, false) else if (dim == 2) PLAN_BALL(2, false) else PLAN_BALL(3, false)
    WLSQM_HIP_CHECK(hipGetLastError());
    size_t scan_bytes = 0, max_bytes = 0;
    WLSQM_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, d_cnt.as<long long>(), P.d_off.as<long long>(), (int)(nx + 1), s));
    WLSQM_HIP_CHECK(hipcub::DeviceReduce::Max(nullptr, max_bytes, d_cnt.as<long long>(), d_max.as<long long>(), (int)nx, s));
    if ((rc = d_tmp.alloc(std::max<size_t>(std::max(scan_bytes, max_bytes), 16)))) return rc;
    WLSQM_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, scan_bytes, d_cnt.as<long long>(), P.d_off.as<long long>(), (int)(nx + 1), s));
    WLSQM_HIP_CHECK(hipcub::DeviceReduce::Max(d_tmp.p, max_bytes, d_cnt.as<long long>(), d_max.as<long long>(), (int)nx, s));
    long long h_n = 0, h_max = 0;
    WLSQM_HIP_CHECK(hipMemcpyAsync(&h_n, P.d_off.as<long long>() + nx, 8, hipMemcpyDeviceToHost, s));
    WLSQM_HIP_CHECK(hipMemcpyAsync(&h_max, d_max.p, 8, hipMemcpyDeviceToHost, s));
    WLSQM_HIP_CHECK(hipStreamSynchronize(s));
    P.nlist = h_n; P.max_list = h_max;
    if ((rc = P.d_idx.alloc((size_t)std::max<long long>(h_n, 1) * 4))) {
        if (rc == WLSQM_EMEMORY) set_error("the neighbour lists of the interpolation plan do not fit the device memory");
        return rc;
    }
    if (dim == 1) PLAN_BALL(1, true) else if (dim == 2) PLAN_BALL(2, true) else PLAN_BALL(3, true)
#undef PLAN_BALL
    WLSQM_HIP_CHECK(hipGetLastError());
    WLSQM_HIP_CHECK(hipStreamSynchronize(s));      // the grid and the counts die with this scope
    return WLSQM_OK;
}

static int plan_create(wlsqm_interp_plan** out, int device, hipStream_t s, int dimension, int64_t nmodels, const double* xi,
                       int64_t xi_stride, const int32_t* order, int64_t order_stride, int mode, const double* x, int64_t x_stride,
                       int64_t nx, double r, const int64_t* I) {
    if (!out) { set_error("null out"); return WLSQM_EVALUE; }
    *out = nullptr;
    if (dimension < 1 || dimension > 3) { set_error("Dimension must be 1, 2 or 3"); return WLSQM_EVALUE; }
    if (nmodels < 1 || nmodels > 0x7fffffffLL) { set_error("1 .. 2^31 - 1 models"); return WLSQM_EVALUE; }
    if (nx < 0 || nx >= 0x7fffffffLL) { set_error("0 .. 2^31 - 2 evaluation points"); return WLSQM_EVALUE; }
    if (mode != 0 && mode != 1) { set_error("mode must be 0 (nearest) or 1 (continuous)"); return WLSQM_EVALUE; }
    if (mode == 1 && !(r > 0.0)) { set_error("r must be positive"); return WLSQM_EVALUE; }
    if (mode == 1 && I) { set_error("I names the model per point in nearest mode only"); return WLSQM_EVALUE; }
    if (!xi || !order || (!x && nx > 0)) { set_error("null array"); return WLSQM_EVALUE; }
    if (xi_stride < dimension || (nx > 0 && x_stride < dimension) || (order_stride != 0 && order_stride < 1)) {
        set_error("xi / x rows must hold `dimension` contiguous coordinates; order_stride must be 0 or positive"); return WLSQM_EVALUE;
    }
    DeviceScope scope; int rc = scope.enter(device);
    if (rc != WLSQM_OK) return rc;
    wlsqm_interp_plan* P = new (std::nothrow) wlsqm_interp_plan();
    if (!P) { set_error("out of memory"); return WLSQM_EMEMORY; }
    struct Guard { wlsqm_interp_plan* p; ~Guard() { delete p; } } guard{P};      // freed on every early return (the device is current)
    P->device = device; P->dimension = dimension; P->mode = mode; P->nmodels = nmodels; P->nx = nx; P->r = mode == 1 ? r : 0.0;
    DevBuf d_flags;
    if ((rc = P->d_xi.alloc((size_t)nmodels * dimension * 8)) || (rc = P->d_order.alloc((size_t)nmodels * 4)) ||
        (rc = P->d_x.alloc((size_t)std::max<int64_t>(nx, 1) * dimension * 8)) || (rc = d_flags.alloc(8))) return rc;
    WLSQM_HIP_CHECK(hipMemsetAsync(d_flags.p, 0, 8, s));
    hipLaunchKernelGGL(interp_plan_pack_rows_kernel, dim3(blocks_of(nmodels, 256)), dim3(256), 0, s, xi, (long long)xi_stride,
                       (long long)nmodels, dimension, P->d_xi.as<double>());
    hipLaunchKernelGGL(interp_plan_pack_order_kernel, dim3(blocks_of(nmodels, 256)), dim3(256), 0, s, order, (long long)order_stride,
                       (long long)nmodels, P->d_order.as<int>(), d_flags.as<int>());
    if (nx > 0)
        hipLaunchKernelGGL(interp_plan_pack_rows_kernel, dim3(blocks_of(nx, 256)), dim3(256), 0, s, x, (long long)x_stride,
                           (long long)nx, dimension, P->d_x.as<double>());
    WLSQM_HIP_CHECK(hipGetLastError());
    int h_flags[2] = {0, 0};
    WLSQM_HIP_CHECK(hipMemcpyAsync(h_flags, d_flags.p, 8, hipMemcpyDeviceToHost, s));
    WLSQM_HIP_CHECK(hipStreamSynchronize(s));
    if (h_flags[0]) { set_error("order must be 0, 1, 2, 3 or 4"); return WLSQM_EVALUE; }
    P->max_order = h_flags[1];
    if (mode == 0) {
        if ((rc = P->d_I.alloc((size_t)std::max<int64_t>(nx, 1) * 8))) return rc;
        if (I && nx > 0) {
            WLSQM_HIP_CHECK(hipMemcpyAsync(P->d_I.p, I, (size_t)nx * 8, hipMemcpyDeviceToDevice, s));
            WLSQM_HIP_CHECK(hipStreamSynchronize(s));
        } else if ((rc = nearest_search(dimension, nmodels, P->d_xi.as<double>(), nx, P->d_x.as<double>(), dimension,
                                        P->d_I.as<long long>(), s))) return rc;
    } else if ((rc = build_lists(*P, s))) return rc;
    guard.p = nullptr;
    *out = P;
    return WLSQM_OK;
}

template <int DIM, int MAXORD>
static void launch_eval(const wlsqm_interp_plan& P, const PlanEval& q, const PlanDiffs& D, hipStream_t s) {
    const unsigned blocks = blocks_of(q.nx, 256);
    if (P.mode == 0) hipLaunchKernelGGL((interp_plan_eval_kernel<DIM, MAXORD, false>), dim3(blocks), dim3(256), 0, s, q, D);
    else hipLaunchKernelGGL((interp_plan_eval_kernel<DIM, MAXORD, true>), dim3(blocks), dim3(256), 0, s, q, D);
}

// The inverted index of the adjoint: a stable radix sort of the (model, point) pairs by model, so that the entries of a model are in
// ascending point number and the index is a function of the inputs alone; offsets by binary search in the sorted keys; the models with
// more than kAdjointLong entries compacted in ascending model number.  Continuous plans also get W[nx].  Synchronises `s`.
static int build_adjoint_index(wlsqm_interp_plan& P, hipStream_t s) {
    int rc;
    const int dim = P.dimension;
    const long long nx = P.nx, nmodels = P.nmodels, n = P.mode == 0 ? nx : P.nlist;
    if (n > 0x7fffffffLL) { set_error("the adjoint's inverted index holds at most 2^31 - 1 entries"); return WLSQM_EVALUE; }
    if ((rc = P.d_toff.alloc((size_t)(nmodels + 1) * 8)) || (rc = P.d_tpt.alloc((size_t)std::max<long long>(n, 1) * 4))) return rc;
    if (P.mode == 1) {
        if ((rc = P.d_W.alloc((size_t)std::max<long long>(nx, 1) * 8))) return rc;
        if (nx > 0) {
#define PLAN_W(D)                                                                                                                \
    hipLaunchKernelGGL((interp_plan_weight_sum_kernel<D>), dim3(blocks_of(nx, 256)), dim3(256), 0, s, P.d_xi.as<double>(),       \
                       P.d_x.as<double>(), nx, P.d_off.as<long long>(), P.d_idx.as<int>(), P.r * P.r, P.d_W.as<double>());
            if (dim == 1) PLAN_W(1) else if (dim == 2) PLAN_W(2) else PLAN_W(3)
#undef PLAN_W
            WLSQM_HIP_CHECK(hipGetLastError());
        }
    }
    if (n == 0) {
        WLSQM_HIP_CHECK(hipMemsetAsync(P.d_toff.p, 0, P.d_toff.n, s));
        if ((rc = P.d_long.alloc(4))) return rc;
        WLSQM_HIP_CHECK(hipStreamSynchronize(s));
        P.adj_entries = P.adj_max_len = P.adj_nlong = 0;
        P.adj_ready = true;
        return WLSQM_OK;
    }
    DevBuf d_key, d_val, d_skey, d_len, d_flag, d_pos, d_max, d_tmp;
    if ((rc = d_key.alloc((size_t)n * 4)) || (rc = d_val.alloc((size_t)n * 4)) || (rc = d_skey.alloc((size_t)n * 4)) ||
        (rc = d_len.alloc((size_t)(nmodels + 1) * 8)) || (rc = d_flag.alloc((size_t)(nmodels + 1) * 8)) ||
        (rc = d_pos.alloc((size_t)(nmodels + 1) * 8)) || (rc = d_max.alloc(8))) return rc;
    if (P.mode == 0)
        hipLaunchKernelGGL(interp_plan_pairs_nearest_kernel, dim3(blocks_of(nx, 256)), dim3(256), 0, s, P.d_I.as<long long>(), nx, nmodels,
                           d_key.as<unsigned>(), d_val.as<int>());
    else
        hipLaunchKernelGGL(interp_plan_pairs_lists_kernel, dim3(blocks_of(nx, 256)), dim3(256), 0, s, P.d_off.as<long long>(),
                           P.d_idx.as<int>(), nx, d_key.as<unsigned>(), d_val.as<int>());
    WLSQM_HIP_CHECK(hipGetLastError());
    int end_bit = 1;                                             // the keys are 0 .. nmodels
    while (end_bit < 32 && (1ull << end_bit) <= (unsigned long long)nmodels) ++end_bit;
    size_t sort_bytes = 0, scan_bytes = 0, max_bytes = 0;
    WLSQM_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, d_key.as<unsigned>(), d_skey.as<unsigned>(), d_val.as<int>(),
                                                       P.d_tpt.as<int>(), (int)n, 0, end_bit, s));
    WLSQM_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, d_flag.as<long long>(), d_pos.as<long long>(), (int)(nmodels + 1), s));
    WLSQM_HIP_CHECK(hipcub::DeviceReduce::Max(nullptr, max_bytes, d_len.as<long long>(), d_max.as<long long>(), (int)nmodels, s));
    if ((rc = d_tmp.alloc(std::max<size_t>(std::max(sort_bytes, std::max(scan_bytes, max_bytes)), 16)))) return rc;
    WLSQM_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(d_tmp.p, sort_bytes, d_key.as<unsigned>(), d_skey.as<unsigned>(), d_val.as<int>(),
                                                       P.d_tpt.as<int>(), (int)n, 0, end_bit, s));
    hipLaunchKernelGGL(interp_plan_offsets_kernel, dim3(blocks_of(nmodels + 1, 256)), dim3(256), 0, s, d_skey.as<unsigned>(), n, nmodels,
                       P.d_toff.as<long long>());
    hipLaunchKernelGGL(interp_plan_lengths_kernel, dim3(blocks_of(nmodels + 1, 256)), dim3(256), 0, s, P.d_toff.as<long long>(), nmodels,
                       d_len.as<long long>(), d_flag.as<long long>());
    WLSQM_HIP_CHECK(hipGetLastError());
    WLSQM_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, scan_bytes, d_flag.as<long long>(), d_pos.as<long long>(), (int)(nmodels + 1), s));
    WLSQM_HIP_CHECK(hipcub::DeviceReduce::Max(d_tmp.p, max_bytes, d_len.as<long long>(), d_max.as<long long>(), (int)nmodels, s));
    long long h_n = 0, h_max = 0, h_long = 0;
    WLSQM_HIP_CHECK(hipMemcpyAsync(&h_n, P.d_toff.as<long long>() + nmodels, 8, hipMemcpyDeviceToHost, s));
    WLSQM_HIP_CHECK(hipMemcpyAsync(&h_max, d_max.p, 8, hipMemcpyDeviceToHost, s));
    WLSQM_HIP_CHECK(hipMemcpyAsync(&h_long, d_pos.as<long long>() + nmodels, 8, hipMemcpyDeviceToHost, s));
    WLSQM_HIP_CHECK(hipStreamSynchronize(s));
    if ((rc = P.d_long.alloc((size_t)std::max<long long>(h_long, 1) * 4))) return rc;
    if (h_long > 0) {
        hipLaunchKernelGGL(interp_plan_compact_long_kernel, dim3(blocks_of(nmodels, 256)), dim3(256), 0, s, d_len.as<long long>(),
                           d_pos.as<long long>(), nmodels, P.d_long.as<int>());
        WLSQM_HIP_CHECK(hipGetLastError());
    }
    WLSQM_HIP_CHECK(hipStreamSynchronize(s));                    // the sort's buffers die with this scope
    P.adj_entries = h_n; P.adj_max_len = h_max; P.adj_nlong = h_long;
    P.adj_ready = true;
    return WLSQM_OK;
}

template <int DIM, int MAXORD>
static void launch_adjoint(const wlsqm_interp_plan& P, const PlanAdj& q, const PlanDiffs& D, hipStream_t s) {
    const unsigned blocks = blocks_of(q.nmodels, 256), wblocks = blocks_of(q.nlong, 4);
    if (P.mode == 0) {
        hipLaunchKernelGGL((interp_plan_adjoint_lane_kernel<DIM, MAXORD, false>), dim3(blocks), dim3(256), 0, s, q, D);
        if (q.nlong > 0) hipLaunchKernelGGL((interp_plan_adjoint_wave_kernel<DIM, MAXORD, false>), dim3(wblocks), dim3(256), 0, s, q, D);
    } else {
        hipLaunchKernelGGL((interp_plan_adjoint_lane_kernel<DIM, MAXORD, true>), dim3(blocks), dim3(256), 0, s, q, D);
        if (q.nlong > 0) hipLaunchKernelGGL((interp_plan_adjoint_wave_kernel<DIM, MAXORD, true>), dim3(wblocks), dim3(256), 0, s, q, D);
    }
}

extern "C" {

int wlsqm_hip_interp_plan_create(wlsqm_interp_plan** out, int device, void* stream, int dimension, int64_t nmodels,
                                 const double* xi_dev, int64_t xi_stride, const int32_t* order_dev, int64_t order_stride,
                                 int mode, const double* x_dev, int64_t x_stride, int64_t nx, double r, const int64_t* I_dev) {
    return plan_create(out, device, (hipStream_t)stream, dimension, nmodels, xi_dev, xi_stride, order_dev, order_stride, mode, x_dev,
                       x_stride, nx, r, I_dev);
}

int wlsqm_hip_interp_plan_create_expert(wlsqm_interp_plan** out, wlsqm_expert* h, void* stream, int mode,
                                        const double* x_dev, int64_t x_stride, int64_t nx, double r, const int64_t* I_dev) {
    if (out) *out = nullptr;
    ExpertView v{};
    int rc = expert_view(h, &v);
    if (rc != WLSQM_OK) return rc;
    if (!v.ready) { set_error("Solver is not in the ready state; prepare() must be called before interpolation_plan()"); return WLSQM_ERUNTIME; }
    return plan_create(out, v.device, (hipStream_t)stream, v.dimension, v.nmodels, v.xi, v.dimension, v.order, 1, mode, x_dev,
                       x_stride, nx, r, I_dev);
}

int wlsqm_hip_interp_plan_info(const wlsqm_interp_plan* P, int64_t* nx, int64_t* nlist, int64_t* max_list, int64_t* bytes) {
    if (!P) { set_error("null plan"); return WLSQM_EVALUE; }
    if (nx) *nx = P->nx;
    if (nlist) *nlist = P->nlist;
    if (max_list) *max_list = P->max_list;
    if (bytes) *bytes = P->bytes();
    return WLSQM_OK;
}

int wlsqm_hip_interp_plan_export(const wlsqm_interp_plan* P, void* stream, int64_t* I_or_off_dev, int64_t* idx_dev) {
    if (!P || !I_or_off_dev) { set_error("null argument"); return WLSQM_EVALUE; }
    DeviceScope scope; int rc = scope.enter(P->device);
    if (rc != WLSQM_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (P->mode == 0) {
        if (P->nx > 0) WLSQM_HIP_CHECK(hipMemcpyAsync(I_or_off_dev, P->d_I.p, (size_t)P->nx * 8, hipMemcpyDeviceToDevice, s));
        return WLSQM_OK;
    }
    WLSQM_HIP_CHECK(hipMemcpyAsync(I_or_off_dev, P->d_off.p, (size_t)(P->nx + 1) * 8, hipMemcpyDeviceToDevice, s));
    if (P->nlist > 0) {
        if (!idx_dev) { set_error("null argument"); return WLSQM_EVALUE; }
        hipLaunchKernelGGL(interp_plan_widen_kernel, dim3(blocks_of(P->nlist, 256)), dim3(256), 0, s, P->d_idx.as<int>(),
                           (long long)P->nlist, reinterpret_cast<long long*>(idx_dev));
        WLSQM_HIP_CHECK(hipGetLastError());
    }
    return WLSQM_OK;
}

int wlsqm_hip_interp_plan_eval_device(const wlsqm_interp_plan* P, void* stream, int64_t nfields,
                                      const double* fi_dev, int64_t fi_stride_field, int64_t fi_stride_model,
                                      const int32_t* diffs, int ndiff, double* out_dev, int64_t out_stride_field,
                                      int64_t out_stride_diff) {
    if (!P) { set_error("null plan"); return WLSQM_EVALUE; }
    if (ndiff < 0 || ndiff > 35) { set_error("at most 35 diffs per call"); return WLSQM_EVALUE; }
    if (nfields < 0) { set_error("nfields must be >= 0"); return WLSQM_EVALUE; }
    if (P->nx == 0 || ndiff == 0 || nfields == 0) return WLSQM_OK;
    if (!fi_dev || !diffs || !out_dev) { set_error("null argument"); return WLSQM_EVALUE; }
    DeviceScope scope; int rc = scope.enter(P->device);
    if (rc != WLSQM_OK) return rc;
    // instantiations for the plan's largest order rounded up to 2 or 4: the registers of the 35 derivatives of 3D order 4 are not
    // spent on an order-2 plan
    const int maxord = P->max_order <= 2 ? 2 : 4;
    const int no = ndofs(P->dimension, maxord);
    PlanDiffs D{};
    D.n = ndiff;
    for (int j = 0; j < ndiff; ++j) D.d[j] = (diffs[j] >= 0 && diffs[j] < no) ? diffs[j] : -1;
    PlanEval q{};
    q.xi = P->d_xi.as<double>(); q.order = P->d_order.as<int>(); q.nmodels = P->nmodels;
    q.x = P->d_x.as<double>(); q.nx = P->nx;
    q.I = P->d_I.as<long long>(); q.off = P->d_off.as<long long>(); q.idx = P->d_idx.as<int>(); q.r2 = P->r * P->r;
    q.fi = fi_dev; q.sfi_f = fi_stride_field; q.sfi_m = fi_stride_model; q.nfields = nfields;
    q.out = out_dev; q.so_f = out_stride_field; q.so_d = out_stride_diff;
    hipStream_t s = (hipStream_t)stream;
    if (P->dimension == 1) { if (maxord == 2) launch_eval<1, 2>(*P, q, D, s); else launch_eval<1, 4>(*P, q, D, s); }
    else if (P->dimension == 2) { if (maxord == 2) launch_eval<2, 2>(*P, q, D, s); else launch_eval<2, 4>(*P, q, D, s); }
    else { if (maxord == 2) launch_eval<3, 2>(*P, q, D, s); else launch_eval<3, 4>(*P, q, D, s); }
    WLSQM_HIP_CHECK(hipGetLastError());
    return WLSQM_OK;
}

int wlsqm_hip_interp_plan_eval_expert(const wlsqm_interp_plan* P, wlsqm_expert* h, void* stream, const int32_t* diffs, int ndiff,
                                      double* out_dev, int64_t out_stride_diff) {
    if (!P) { set_error("null plan"); return WLSQM_EVALUE; }
    ExpertView v{};
    int rc = expert_view(h, &v);
    if (rc != WLSQM_OK) return rc;
    if (v.device != P->device || v.dimension != P->dimension || v.nmodels != P->nmodels) {
        set_error("the solver is not the one the plan was made for (device, dimension or number of cases differ)"); return WLSQM_EVALUE;
    }
    if (!v.solved || !v.fi) { set_error("the solver has not solved yet: no coefficients to evaluate"); return WLSQM_ERUNTIME; }
    return wlsqm_hip_interp_plan_eval_device(P, stream, 1, v.fi, 0, v.sfi, diffs, ndiff, out_dev, 0, out_stride_diff);
}

int wlsqm_hip_interp_plan_prepare_adjoint(wlsqm_interp_plan* P, void* stream, int* built) {
    if (built) *built = 0;
    if (!P) { set_error("null plan"); return WLSQM_EVALUE; }
    if (!P->adj_ready) {
        DeviceScope scope; int rc = scope.enter(P->device);
        if (rc != WLSQM_OK) return rc;
        if ((rc = build_adjoint_index(*P, (hipStream_t)stream))) return rc;
    }
    if (built) *built = 1;                                       // the index exists afterwards
    return WLSQM_OK;
}

int wlsqm_hip_interp_plan_adjoint_info(const wlsqm_interp_plan* P, int64_t* nentries, int64_t* max_len, int64_t* nlong,
                                       int32_t* threshold) {
    if (!P) { set_error("null plan"); return WLSQM_EVALUE; }
    if (nentries) *nentries = P->adj_ready ? P->adj_entries : -1;
    if (max_len) *max_len = P->adj_ready ? P->adj_max_len : -1;
    if (nlong) *nlong = P->adj_ready ? P->adj_nlong : -1;
    if (threshold) *threshold = kAdjointLong;
    return WLSQM_OK;
}

int wlsqm_hip_interp_plan_export_transposed(const wlsqm_interp_plan* P, void* stream, int64_t* toff_dev, int64_t* tpt_dev) {
    if (!P || !toff_dev) { set_error("null argument"); return WLSQM_EVALUE; }
    if (!P->adj_ready) { set_error("the plan has no inverted index yet: call prepare_adjoint first"); return WLSQM_ERUNTIME; }
    DeviceScope scope; int rc = scope.enter(P->device);
    if (rc != WLSQM_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    WLSQM_HIP_CHECK(hipMemcpyAsync(toff_dev, P->d_toff.p, (size_t)(P->nmodels + 1) * 8, hipMemcpyDeviceToDevice, s));
    if (P->adj_entries > 0) {
        if (!tpt_dev) { set_error("null argument"); return WLSQM_EVALUE; }
        hipLaunchKernelGGL(interp_plan_widen_kernel, dim3(blocks_of(P->adj_entries, 256)), dim3(256), 0, s, P->d_tpt.as<int>(),
                           (long long)P->adj_entries, reinterpret_cast<long long*>(tpt_dev));
        WLSQM_HIP_CHECK(hipGetLastError());
    }
    return WLSQM_OK;
}

int wlsqm_hip_interp_plan_eval_adjoint_device(wlsqm_interp_plan* P, void* stream, int64_t nfields, const int32_t* diffs, int ndiff,
                                              const double* g_dev, int64_t g_stride_field, int64_t g_stride_diff,
                                              double* grad_fi_dev, int64_t gfi_stride_field, int64_t gfi_stride_model, int ncols) {
    if (!P) { set_error("null plan"); return WLSQM_EVALUE; }
    if (ndiff < 0 || ndiff > 35) { set_error("at most 35 diffs per call"); return WLSQM_EVALUE; }
    if (nfields < 0) { set_error("nfields must be >= 0"); return WLSQM_EVALUE; }
    if (ncols < ndofs(P->dimension, P->max_order)) {
        set_error("grad_fi rows narrower than the number of DOFs of the plan's largest order"); return WLSQM_EVALUE;
    }
    if (gfi_stride_model < ncols) { set_error("grad_fi rows overlap: gfi_stride_model < ncols"); return WLSQM_EVALUE; }
    if (nfields == 0) return WLSQM_OK;
    if (!grad_fi_dev || (ndiff > 0 && !diffs) || (ndiff > 0 && P->nx > 0 && !g_dev)) { set_error("null argument"); return WLSQM_EVALUE; }
    DeviceScope scope; int rc = scope.enter(P->device);
    if (rc != WLSQM_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (!P->adj_ready) {
        // built on demand (it synchronises), never while the stream is capturing: checked before anything is enqueued
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
        if (cap != hipStreamCaptureStatusNone) {
            set_error("the plan has no inverted index yet and the stream is capturing: call prepare_adjoint before the capture");
            return WLSQM_ERUNTIME;
        }
        if ((rc = build_adjoint_index(*P, s))) return rc;
    }
    const int maxord = P->max_order <= 2 ? 2 : 4;                // the forward's instantiations
    const int no = ndofs(P->dimension, maxord);
    PlanDiffs D{};
    D.n = ndiff;
    for (int j = 0; j < ndiff; ++j) D.d[j] = (diffs[j] >= 0 && diffs[j] < no) ? diffs[j] : -1;
    PlanAdj q{};
    q.xi = P->d_xi.as<double>(); q.order = P->d_order.as<int>(); q.nmodels = P->nmodels;
    q.x = P->d_x.as<double>();
    q.toff = P->d_toff.as<long long>(); q.tpt = P->d_tpt.as<int>(); q.W = P->d_W.as<double>(); q.r2 = P->r * P->r;
    q.longs = P->d_long.as<int>(); q.nlong = P->adj_nlong;
    q.g = g_dev; q.sg_f = g_stride_field; q.sg_d = g_stride_diff; q.nfields = nfields;
    q.gfi = grad_fi_dev; q.sgfi_f = gfi_stride_field; q.sgfi_m = gfi_stride_model; q.ncols = ncols;
    if (P->dimension == 1) { if (maxord == 2) launch_adjoint<1, 2>(*P, q, D, s); else launch_adjoint<1, 4>(*P, q, D, s); }
    else if (P->dimension == 2) { if (maxord == 2) launch_adjoint<2, 2>(*P, q, D, s); else launch_adjoint<2, 4>(*P, q, D, s); }
    else { if (maxord == 2) launch_adjoint<3, 2>(*P, q, D, s); else launch_adjoint<3, 4>(*P, q, D, s); }
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel(P->adj_nlong > 0 ? "interp-plan-adjoint+wave" : "interp-plan-adjoint");
    return WLSQM_OK;
}

int wlsqm_hip_interp_plan_destroy(wlsqm_interp_plan* P) {
    if (!P) return WLSQM_OK;
    DeviceScope scope;
    (void)scope.enter(P->device);
    delete P;
    return WLSQM_OK;
}

}  // extern "C"
