// krylov.hip — implicit solves with a stencil operator: BiCGSTAB on M = diag(d) + c A, A one value plane of a square SELL-64 matrix
// (the layout is stated in include/wlsqm_hip.h), with an optional Jacobi preconditioner, resident on the device.
//
// The state of a solve is one block of scalars in device memory (KrylovScalars): every kernel reads it at its head and returns at once,
// wave-uniformly, when `done` is set, so any number of iterations can be enqueued behind a solve that has stopped.  It is written by one
// lane of the one-workgroup reduce kernel, in plain stores.  The host reads it only when the caller asks.
//
// The product is sell_block<1, 1>'s statement (csrc/stencil.hip): one wave per slice, one lane per row, the entries in order with fma, the
// padding under the lane's predicate and never loaded.  The same pass forms the workgroup's partials of the dot products of the step.
// Dot products: one product per lane (no contraction), the wave's 64 lanes through a fixed tree (lane l += lane l + 32, 16, ... 1), the
// workgroup's four waves in order, one partial per workgroup; the reduce kernel (one workgroup) sums partials t, t + 256, ... in thread t,
// then the same tree and wave order.  No atomics: the bits are a function of the inputs, not of the launch.
#include "wlsqm_dispatch.hpp"

#pragma clang fp contract(off)      // a * b + c below is two roundings; the fused sums are __builtin_fma

namespace wlsqm {

struct KrylovScalars {              // 128 bytes at the head of the workspace; wlsqm/hip.py reads it as 8 doubles and 4 int32
    double rho, rho_old, alpha, omega;
    double rr, stop;                // (r, r) of the recursive residual; the threshold max(rtol ||b||, atol) on its root
    double dot0, dot1;              // wlsqm_hip_krylov_product_device's results; dot0 also wlsqm_hip_krylov_grads_device's dL/dscale
    int iterations, status, done, maxiter;
    double pad[6];
};

constexpr int KRYLOV_RUNNING = -1;
enum { KRYLOV_CONVERGED = 0, KRYLOV_MAXITER = 1, KRYLOV_BREAKDOWN = 2, KRYLOV_NONFINITE = 3, KRYLOV_DIAGONAL = 4 };
constexpr long long KRYLOV_HEAD = sizeof(KrylovScalars) / sizeof(double);
constexpr int KRYLOV_VECTORS = 9;   // r, r0, p, v, s, t, phat, shat, dinv

struct KrylovSys {                  // M = diag(d) + c A
    long long nrows;
    const int32_t* len; const int32_t* width; const long long* soff;
    const int32_t* col; const double* val;
    const double* dvec; double dconst, c;                       // d_i = dvec ? dvec[i] : dconst
};

struct KrylovWork {
    KrylovScalars* sc; double* partial; long long nwg;          // partial: 2 planes of nwg
    double *r, *r0, *p, *v, *s, *t, *phat, *shat, *dinv;
};

static KrylovWork krylov_work(void* workspace, long long nrows, bool jacobi) {
    KrylovWork w;
    double* base = static_cast<double*>(workspace);
    w.sc = static_cast<KrylovScalars*>(workspace);
    w.nwg = (nrows + 255) / 256;
    w.partial = base + KRYLOV_HEAD;
    double* vec = w.partial + 2 * w.nwg;
    w.r = vec; w.r0 = vec + nrows; w.p = vec + 2 * nrows; w.v = vec + 3 * nrows; w.s = vec + 4 * nrows; w.t = vec + 5 * nrows;
    // without a preconditioner phat is p and shat is s: nothing is copied
    w.phat = jacobi ? vec + 6 * nrows : w.p; w.shat = jacobi ? vec + 7 * nrows : w.s; w.dinv = jacobi ? vec + 8 * nrows : nullptr;
    return w;
}

// The sums a and b of the workgroup's 256 lanes into partial[blockIdx.x] and partial[nwg + blockIdx.x] (b only when TWO): the fixed tree.
template <bool TWO>
__device__ __forceinline__ void block_sums(double a, double b, double* partial, long long nwg) {
    __shared__ double part[2][4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off, 64);
        if (TWO) b += __shfl_down(b, off, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { part[0][wave] = a; if (TWO) part[1][wave] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = ((part[0][0] + part[0][1]) + part[0][2]) + part[0][3];
        if (TWO) partial[nwg + blockIdx.x] = ((part[1][0] + part[1][1]) + part[1][2]) + part[1][3];
    }
}

// sum_{e < n} val * x[col] of this lane's row, in entry order with fma: sell_block<1, 1> of csrc/stencil.hip.
__device__ __forceinline__ double krylov_row_sum(const int32_t* col, const double* val, const double* x, int wid, int n) {
    constexpr int UNROLL = 8;
    double acc = 0.0;
    for (int e = 0; e < wid; e += UNROLL) {                      // wave-uniform
        if (e + UNROLL <= n) {
            double xs[UNROLL], vs[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const long long c = col[64LL * (e + u)];
                xs[u] = x[c];
                vs[u] = val[64LL * (e + u)];
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) acc = __builtin_fma(vs[u], xs[u], acc);
        } else {
            for (int u = 0; u < UNROLL && e + u < n; ++u) {
                const long long c = col[64LL * (e + u)];
                acc = __builtin_fma(val[64LL * (e + u)], x[c], acc);
            }
        }
    }
    return acc;
}

enum { SPMV_RESIDUAL = 0, SPMV_V = 1, SPMV_T = 2 };

// y = M in, y_i = fma(c, sum, d_i in_i).
//   SPMV_RESIDUAL: out = out2 = b - y (w is b), partials (out, out) and (b, b)
//   SPMV_V:        out = y, partial (w, out)
//   SPMV_T:        out = y, partials (out, w) and (out, out)
template <int MODE>
__global__ void __launch_bounds__(256) krylov_spmv_kernel(const KrylovSys m, const double* in, const double* w, double* out, double* out2,
                                                          double* partial, const KrylovScalars* sc, int always) {
    if (!always && sc->done) return;                             // uniform: the whole grid
    const int lane = threadIdx.x & 63;
    const long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long row = s * 64 + lane;
    double a = 0.0, b = 0.0;
    if (s * 64 < m.nrows) {                                      // wave-uniform
        const int wid = __builtin_amdgcn_readfirstlane(m.width[s]);
        const long long at = m.soff[s] + lane;
        int n = row < m.nrows ? m.len[row] : 0;
        n = n < wid ? n : wid;
        const double sum = krylov_row_sum(m.col + at, m.val + at, in, wid, n);
        if (row < m.nrows) {
            const double d = m.dvec ? m.dvec[row] : m.dconst;
            const double y = __builtin_fma(m.c, sum, d * in[row]);
            if (MODE == SPMV_RESIDUAL) {
                const double bi = w[row], r = bi - y;
                out[row] = r; out2[row] = r;
                a = r * r; b = bi * bi;
            } else {
                out[row] = y;
                a = w[row] * y;
                if (MODE == SPMV_T) b = y * y;
            }
        }
    }
    block_sums<MODE != SPMV_V>(a, b, partial, gridDim.x);
}

// dinv_i = 1 / (d_i + c * sum_{col = i} val), the sum in entry order; the partial counts the rows whose diagonal is zero or not finite.
__global__ void __launch_bounds__(256) krylov_diag_kernel(const KrylovSys m, double* dinv, double* partial) {
    const int lane = threadIdx.x & 63;
    const long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long row = s * 64 + lane;
    double bad = 0.0;
    if (s * 64 < m.nrows) {                                      // wave-uniform
        const int wid = __builtin_amdgcn_readfirstlane(m.width[s]);
        const long long at = m.soff[s] + lane;
        int n = row < m.nrows ? m.len[row] : 0;
        n = n < wid ? n : wid;
        double sum = 0.0;
        for (int e = 0; e < wid; ++e)                            // wave-uniform
            if (e < n && m.col[at + 64LL * e] == row) sum += m.val[at + 64LL * e];
        if (row < m.nrows) {
            const double diag = (m.dvec ? m.dvec[row] : m.dconst) + m.c * sum;
            const bool ok = diag != 0.0 && __builtin_isfinite(diag);
            dinv[row] = ok ? 1.0 / diag : 0.0;
            bad = ok ? 0.0 : 1.0;
        }
    }
    block_sums<false>(bad, 0.0, partial, gridDim.x);
}

// The gradients of a loss through the solve M x = b, lam the solution of M^T lam = dL/dx, in one pass over the
// forward matrix with krylov_spmv_kernel's mapping.  Each output is a template flag, so a pass without SCALE never loads val and a
// pass without VALUES never stores into a plane:
//   VALUES: gval[at + 64 e] = -(t * x[col]) with t = c * lam_j, two roundings, for the live entries of row j; +0.0 in every padding
//           position of the slice, the lanes of rows beyond nrows included (their padding col is never loaded)
//   DIAG:   gdiag[j] = -(lam_j * x_j)
//   SCALE:  the workgroup's partial of sum_j lam_j * (row j of A) x, the row sum krylov_row_sum's bits (the same fma chain)
template <bool VALUES, bool DIAG, bool SCALE>
__global__ void __launch_bounds__(256) krylov_grads_kernel(const KrylovSys m, const double* lam, const double* x, double* gval,
                                                           double* gdiag, double* partial) {
    const int lane = threadIdx.x & 63;
    const long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long row = s * 64 + lane;
    double a = 0.0;
    if (s * 64 < m.nrows) {                                      // wave-uniform
        const bool live = row < m.nrows;
        const double lj = live ? lam[row] : 0.0;
        if (DIAG && live) gdiag[row] = -(lj * x[row]);
        if (VALUES || SCALE) {
            constexpr int UNROLL = 8;
            const int wid = __builtin_amdgcn_readfirstlane(m.width[s]);
            const long long at = m.soff[s] + lane;
            int n = live ? m.len[row] : 0;
            n = n < wid ? n : wid;
            const int32_t* col = m.col + at;
            const double* val = m.val + at;
            double* out = gval + at;
            const double t = m.c * lj;
            double acc = 0.0;
            for (int e = 0; e < wid; e += UNROLL) {              // wave-uniform
                if (e + UNROLL <= n) {
                    double xs[UNROLL], vs[UNROLL];
#pragma unroll
                    for (int u = 0; u < UNROLL; ++u) {
                        xs[u] = x[col[64LL * (e + u)]];
                        if (SCALE) vs[u] = val[64LL * (e + u)];
                    }
#pragma unroll
                    for (int u = 0; u < UNROLL; ++u) {
                        if (VALUES) out[64LL * (e + u)] = -(t * xs[u]);
                        if (SCALE) acc = __builtin_fma(vs[u], xs[u], acc);
                    }
                } else {
                    for (int u = 0; u < UNROLL && e + u < wid; ++u) {
                        if (e + u < n) {
                            const double xv = x[col[64LL * (e + u)]];
                            if (VALUES) out[64LL * (e + u)] = -(t * xv);
                            if (SCALE) acc = __builtin_fma(val[64LL * (e + u)], xv, acc);
                        } else if (VALUES) {
                            out[64LL * (e + u)] = 0.0;
                        }
                    }
                }
            }
            if (SCALE) a = lj * acc;
        }
    }
    if (SCALE) block_sums<false>(a, 0.0, partial, gridDim.x);
}

enum { UPDATE_P = 0, UPDATE_S = 1, UPDATE_X = 2 };

//   UPDATE_P: p = r + beta (p - omega v) (the first iteration: p = r), phat = dinv p
//   UPDATE_S: s = r - alpha v, shat = dinv s
//   UPDATE_X: x += alpha phat + omega shat, r = s - omega t, partials (r0, r) and (r, r)
template <int MODE>
__global__ void __launch_bounds__(256) krylov_update_kernel(long long nrows, const KrylovWork k, double* x, const KrylovScalars* sc) {
    if (sc->done) return;                                        // uniform: the whole grid
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    double a = 0.0, b = 0.0;
    if (MODE == UPDATE_P) {
        if (i >= nrows) return;
        double p = k.r[i];
        if (sc->iterations > 0) {
            const double omega = sc->omega, beta = (sc->rho / sc->rho_old) * (sc->alpha / omega);
            p = p + beta * (k.p[i] - omega * k.v[i]);
        }
        k.p[i] = p;
        if (k.dinv) k.phat[i] = k.dinv[i] * p;
    } else if (MODE == UPDATE_S) {
        if (i >= nrows) return;
        const double s = k.r[i] - sc->alpha * k.v[i];
        k.s[i] = s;
        if (k.dinv) k.shat[i] = k.dinv[i] * s;
    } else {
        if (i < nrows) {
            const double omega = sc->omega;
            x[i] = x[i] + (sc->alpha * k.phat[i] + omega * k.shat[i]);
            const double r = k.s[i] - omega * k.t[i];
            k.r[i] = r;
            a = k.r0[i] * r; b = r * r;
        }
        block_sums<true>(a, b, k.partial, gridDim.x);
    }
}

enum { REDUCE_DIAG = 0, REDUCE_RESIDUAL = 1, REDUCE_ALPHA = 2, REDUCE_OMEGA = 3, REDUCE_RHO = 4, REDUCE_PRODUCT = 5, REDUCE_NEGATED = 6 };

__device__ __forceinline__ void krylov_stop(KrylovScalars* sc, int status) { sc->status = status; sc->done = 1; }

// The scalar step of `mode` on the sums s0 and s1 of its dot products: one lane.
__device__ __forceinline__ void krylov_scalar_step(int mode, KrylovScalars* sc, double s0, double s1, double rtol, double atol, int maxiter) {
    switch (mode) {
    case REDUCE_DIAG:                                            // the start of a solve: s0 counts the unusable diagonal entries
        sc->rho = sc->rho_old = sc->alpha = sc->omega = 1.0;
        sc->rr = __builtin_nan(""); sc->stop = 0.0;
        sc->iterations = 0; sc->maxiter = maxiter;
        sc->status = s0 != 0.0 ? KRYLOV_DIAGONAL : KRYLOV_RUNNING;
        sc->done = s0 != 0.0 ? 1 : 0;
        break;
    case REDUCE_RESIDUAL: {                                      // s0 = (r, r) = (r0, r), s1 = (b, b)
        sc->rho = s0; sc->rr = s0;
        if (!__builtin_isfinite(s0) || !__builtin_isfinite(s1)) { krylov_stop(sc, KRYLOV_NONFINITE); break; }
        const double rel = rtol * __builtin_sqrt(s1), stop = rel > atol ? rel : atol;
        sc->stop = stop;
        if (__builtin_sqrt(s0) <= stop) krylov_stop(sc, KRYLOV_CONVERGED);
        else if (sc->maxiter <= 0) krylov_stop(sc, KRYLOV_MAXITER);
        break;
    }
    case REDUCE_ALPHA: {                                         // s0 = (r0, v)
        if (!__builtin_isfinite(s0)) { krylov_stop(sc, KRYLOV_NONFINITE); break; }
        if (s0 == 0.0) { krylov_stop(sc, KRYLOV_BREAKDOWN); break; }
        const double alpha = sc->rho / s0;
        if (!__builtin_isfinite(alpha)) { krylov_stop(sc, KRYLOV_NONFINITE); break; }
        sc->alpha = alpha;
        break;
    }
    case REDUCE_OMEGA: {                                         // s0 = (t, s), s1 = (t, t)
        if (!__builtin_isfinite(s0) || !__builtin_isfinite(s1)) { krylov_stop(sc, KRYLOV_NONFINITE); break; }
        const double omega = s1 == 0.0 ? 0.0 : s0 / s1;
        if (!__builtin_isfinite(omega)) { krylov_stop(sc, KRYLOV_NONFINITE); break; }
        sc->omega = omega;
        break;
    }
    case REDUCE_RHO: {                                           // s0 = (r0, r), s1 = (r, r)
        const double rho_old = sc->rho;
        const int it = sc->iterations + 1;
        sc->iterations = it; sc->rho_old = rho_old; sc->rho = s0; sc->rr = s1;
        if (!__builtin_isfinite(s0) || !__builtin_isfinite(s1)) krylov_stop(sc, KRYLOV_NONFINITE);
        else if (__builtin_sqrt(s1) <= sc->stop) krylov_stop(sc, KRYLOV_CONVERGED);
        else if (it >= sc->maxiter) krylov_stop(sc, KRYLOV_MAXITER);
        else if (s0 == 0.0) krylov_stop(sc, KRYLOV_BREAKDOWN);
        else if (!__builtin_isfinite((s0 / rho_old) * (sc->alpha / sc->omega))) krylov_stop(sc, KRYLOV_NONFINITE);   // the next beta
        break;
    }
    case REDUCE_NEGATED:                                         // krylov_grads_kernel's sum: dL/dscale = -(lam, A x)
        sc->dot0 = -s0;
        break;
    default:                                                     // REDUCE_PRODUCT
        sc->dot0 = s0; sc->dot1 = s1;
        break;
    }
}

// One workgroup: the partials of both planes in index order (thread t takes t, t + 256, ...), then the scalar step of `mode` in one lane.
__global__ void __launch_bounds__(256) krylov_reduce_kernel(int mode, const double* partial, long long nwg, int planes, KrylovScalars* sc,
                                                            double rtol, double atol, int maxiter) {
    if (mode != REDUCE_DIAG && mode != REDUCE_PRODUCT && mode != REDUCE_NEGATED && sc->done) return;      // uniform
    __shared__ double sums[2];
    double a = 0.0, b = 0.0;
    for (long long i = threadIdx.x; i < nwg; i += 256) {
        a += partial[i];
        if (planes > 1) b += partial[nwg + i];
    }
    block_sums<true>(a, b, sums, 1);                             // blockIdx.x == 0: sums[0], sums[1]
    if (threadIdx.x != 0) return;
    krylov_scalar_step(mode, sc, sums[0], sums[1], rtol, atol, maxiter);
}

static int krylov_system(const char* who, KrylovSys& m, int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width,
                         const int64_t* soff, const int32_t* col, const double* val, const double* dvec, double dconst, double scale,
                         const void* workspace) {
    if (nrows < 1 || nslices < 0 || nrows > 64 * nslices || (nrows + 255) / 256 > 0x7fffffffLL) {
        set_error(std::string(who) + ": nrows must be 1 .. 64 * nslices");
        return WLSQM_EVALUE;
    }
    if (!len || !width || !soff || !col || !val || !workspace) { set_error(std::string(who) + ": null array"); return WLSQM_EVALUE; }
    m.nrows = nrows;
    m.len = len; m.width = width; m.soff = reinterpret_cast<const long long*>(soff);
    m.col = col; m.val = val;
    m.dvec = dvec; m.dconst = dconst; m.c = scale;
    return WLSQM_OK;
}

static void krylov_reduce(int mode, const KrylovWork& w, long long nwg, int planes, double rtol, double atol, int maxiter, hipStream_t stream) {
    hipLaunchKernelGGL(krylov_reduce_kernel, dim3(1), dim3(256), 0, stream, mode, (const double*)w.partial, nwg, planes, w.sc, rtol, atol, maxiter);
}

template <bool VALUES, bool DIAG, bool SCALE>
static void krylov_grads_launch(const KrylovSys& m, const KrylovWork& k, const double* lam, const double* x, double* gval, double* gdiag,
                                hipStream_t s) {
    hipLaunchKernelGGL((krylov_grads_kernel<VALUES, DIAG, SCALE>), dim3((unsigned)k.nwg), dim3(256), 0, s, m, lam, x, gval, gdiag, k.partial);
}

// ---- the block-Jacobi preconditioner: P = blockdiag(M_BB)^-1, block B the rows B NB .. B NB + NB - 1 -----------
// The inverses live in a plane W of nslices * NB * 64 doubles, W[(slice * NB + j) * 64 + lane] = entry (lane % NB, j) of the inverse of the
// block that holds row slice * 64 + lane: a wave's load of column j is one contiguous run of 512 bytes.  NB divides 64, so a block never
// crosses a slice.  Behind the plane sit ceil(nrows / 256) doubles, the per-workgroup counts of the unusable blocks of the last factor,
// which every start reduces into status 4 (they outlive the iterations, which the workspace's partials do not).

__host__ __device__ static inline long long krylov_plane_doubles(long long nslices, int nb) { return nslices * nb * 64; }

// Step K of krylov_blocks_kernel's elimination and the steps behind it: K is a template parameter so that every register index is a constant.
template <int NB, int K>
__device__ __forceinline__ void krylov_eliminate(double (&a)[NB], double (&inv)[NB], int lane, bool& used, int& step, bool& unusable) {
    if constexpr (K < NB) {
        const double mag = __builtin_fabs(a[K]);
        double key = used ? -1.0 : (mag != mag ? __builtin_inf() : mag);
        int who = lane;
#pragma unroll
        for (int off = 1; off < NB; off <<= 1) {
            const double okey = __shfl_xor(key, off, 64);
            const int owho = __shfl_xor(who, off, 64);
            if (okey > key || (okey == key && owho < who)) { key = okey; who = owho; }
        }
        const double pv = __shfl(a[K], who, 64);
        if (!(pv != 0.0 && __builtin_isfinite(pv))) unusable = true;
        const double pinv = 1.0 / pv, f = a[K];
        const bool mine = lane == who;
        if (mine) { used = true; step = K; }
#pragma unroll
        for (int j = K + 1; j < NB; ++j) {
            const double pj = __shfl(a[j], who, 64) * pinv;
            a[j] = mine ? pj : __builtin_fma(-f, pj, a[j]);
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const double qj = __shfl(inv[j], who, 64) * pinv;
            inv[j] = mine ? qj : __builtin_fma(-f, qj, inv[j]);
        }
        krylov_eliminate<NB, K + 1>(a, inv, lane, used, step, unusable);
    }
}

// One wave per slice, one lane per row.  The lane gathers row `lane % NB` of its diagonal block (duplicate columns summed in entry order,
// as krylov_diag_kernel; rows beyond nrows are identity rows), then the NB lanes of a block invert it by Gauss-Jordan elimination on
// [B | I] with partial pivoting: at step k the pivot is the largest |entry k| among the rows that have not been a pivot yet, the lowest
// row winning a tie, a NaN counting as the largest; its row, scaled by 1 / pivot, travels by cross-lane moves (ds_bpermute) and every
// other row of the block eliminates with fma.  Rows are not swapped while eliminating: the row that was the pivot of step k holds row k
// of the inverse at the end, and one last cross-lane move puts it into lane k.  Every register index is a constant after unrolling.
// A zero or non-finite pivot, or a non-finite entry of the inverse, counts the block as unusable.  WT (nullable) receives the
// transposed inverses in the same layout, counts and all.
template <int NB>
__global__ void __launch_bounds__(256) krylov_blocks_kernel(const KrylovSys m, long long nslices, double* W, double* WT) {
    const int lane = threadIdx.x & 63, l = lane & (NB - 1), b0 = lane - l;
    const long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long row = s * 64 + lane;
    double bad = 0.0;
    if (s * 64 < m.nrows) {                                      // wave-uniform
        const int wid = __builtin_amdgcn_readfirstlane(m.width[s]);
        const long long at = m.soff[s] + lane;
        const bool live = row < m.nrows;
        int n = live ? m.len[row] : 0;
        n = n < wid ? n : wid;
        const long long first = row - l;                         // the block's first row and column
        double a[NB], inv[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) a[j] = 0.0;
        for (int e = 0; e < wid; ++e) {                          // wave-uniform
            if (e < n) {
                const long long t = (long long)m.col[at + 64LL * e] - first;
                if (t >= 0 && t < NB) {
                    const double v = m.val[at + 64LL * e];
#pragma unroll
                    for (int j = 0; j < NB; ++j) a[j] += t == j ? v : 0.0;
                }
            }
        }
        const double d = live ? (m.dvec ? m.dvec[row] : m.dconst) : 1.0;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const double dj = j == l ? d : 0.0;
            a[j] = live ? dj + m.c * a[j] : dj;
            inv[j] = j == l ? 1.0 : 0.0;
        }
        bool used = false, unusable = false;
        int step = 0;
        krylov_eliminate<NB, 0>(a, inv, lane, used, step, unusable);
        int src = lane;
#pragma unroll
        for (int j = 0; j < NB; ++j)
            if (__shfl(step, b0 + j, 64) == l) src = b0 + j;
        double* w = W + (s * NB) * 64 + lane;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            inv[j] = __shfl(inv[j], src, 64);
            if (!__builtin_isfinite(inv[j])) unusable = true;
            w[64LL * j] = inv[j];
        }
        if (WT) {
            double* wt = WT + (s * NB + l) * 64 + b0;            // column l of the transposed block, its rows b0 .. b0 + NB - 1
#pragma unroll
            for (int j = 0; j < NB; ++j) wt[j] = inv[j];
        }
        bad = unusable ? 1.0 : 0.0;
    }
    double* counts = W + krylov_plane_doubles(nslices, NB);
    block_sums<false>(bad, 0.0, counts, gridDim.x);
    if (WT && threadIdx.x == 0) WT[krylov_plane_doubles(nslices, NB) + blockIdx.x] = counts[blockIdx.x];
}

// z_lane = sum_j W[.., j, lane] * v_(first + j), j ascending with fma, v taken from the lanes of the wave that hold it.  Every lane of the
// wave takes part; a lane beyond nrows passes 0, and its own row of W is an identity row.
template <int NB>
__device__ __forceinline__ double krylov_block_apply(const double* w, double v, int lane) {
    const int b0 = lane & ~(NB - 1);
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < NB; ++j) acc = __builtin_fma(w[64LL * j], __shfl(v, b0 + j, 64), acc);
    return acc;
}

// krylov_update_kernel's P and S steps with phat = P p and shat = P s: one launch each, p and s never re-read from memory.
template <int NB, int MODE>
__global__ void __launch_bounds__(256) krylov_update_block_kernel(long long nrows, const KrylovWork k, const double* W, const KrylovScalars* sc) {
    if (sc->done) return;                                        // uniform: the whole grid
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const long long s = i >> 6;
    if (s * 64 >= nrows) return;                                 // wave-uniform
    const bool live = i < nrows;
    double u = 0.0;
    if (live) {
        if (MODE == UPDATE_P) {
            u = k.r[i];
            if (sc->iterations > 0) {
                const double omega = sc->omega, beta = (sc->rho / sc->rho_old) * (sc->alpha / omega);
                u = u + beta * (k.p[i] - omega * k.v[i]);
            }
            k.p[i] = u;
        } else {
            u = k.r[i] - sc->alpha * k.v[i];
            k.s[i] = u;
        }
    }
    const double z = krylov_block_apply<NB>(W + (s * NB) * 64 + lane, u, lane);
    if (live) (MODE == UPDATE_P ? k.phat : k.shat)[i] = z;
}

template <int NB>
__global__ void __launch_bounds__(256) krylov_precondition_kernel(long long nrows, const double* W, const double* v, double* out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const long long s = i >> 6;
    if (s * 64 >= nrows) return;                                 // wave-uniform
    const bool live = i < nrows;
    const double z = krylov_block_apply<NB>(W + (s * NB) * 64 + lane, live ? v[i] : 0.0, lane);
    if (live) out[i] = z;
}

static int krylov_block_size(const char* who, int block, const void* planes) {
    if (block != 8 && block != 16 && block != 32) { set_error(std::string(who) + ": block must be 8, 16 or 32"); return WLSQM_EVALUE; }
    if (!planes) { set_error(std::string(who) + ": null array"); return WLSQM_EVALUE; }
    return WLSQM_OK;
}

template <int NB>
static void krylov_block_iterations(const KrylovSys& m, const KrylovWork& w, const double* W, double* x, int64_t niter, hipStream_t s) {
    const dim3 grid((unsigned)w.nwg);
    const KrylovScalars* sc = w.sc;
    const long long nrows = m.nrows;
    for (int64_t it = 0; it < niter; ++it) {
        hipLaunchKernelGGL((krylov_update_block_kernel<NB, UPDATE_P>), grid, dim3(256), 0, s, nrows, w, W, sc);
        hipLaunchKernelGGL((krylov_spmv_kernel<SPMV_V>), grid, dim3(256), 0, s, m, (const double*)w.phat, (const double*)w.r0, w.v, (double*)nullptr, w.partial, sc, 0);
        krylov_reduce(REDUCE_ALPHA, w, w.nwg, 1, 0.0, 0.0, 0, s);
        hipLaunchKernelGGL((krylov_update_block_kernel<NB, UPDATE_S>), grid, dim3(256), 0, s, nrows, w, W, sc);
        hipLaunchKernelGGL((krylov_spmv_kernel<SPMV_T>), grid, dim3(256), 0, s, m, (const double*)w.shat, (const double*)w.s, w.t, (double*)nullptr, w.partial, sc, 0);
        krylov_reduce(REDUCE_OMEGA, w, w.nwg, 2, 0.0, 0.0, 0, s);
        hipLaunchKernelGGL((krylov_update_kernel<UPDATE_X>), grid, dim3(256), 0, s, nrows, w, x, sc);
        krylov_reduce(REDUCE_RHO, w, w.nwg, 2, 0.0, 0.0, 0, s);
    }
}

// ---- stacked right-hand sides: R <= 8 independent recurrences on one matrix, one pass over it for all of them --
// The solver's own vectors are interleaved at the pitch P (2, 4 or 8, the next one above nfields): v[point * P + field], so that the P
// values of a neighbour are one contiguous load of 8 P bytes.  The caller's b and x stay (nfields, npoints) with any strides.  Every field
// has its own KrylovScalars; the bits of field r are those of the single-field kernels above on b_r, x_r alone: the same lane per row, the
// same fma chain, the same trees, per field.  A field that has stopped is frozen: its stores are predicated off (`frozen`, uniform over
// the grid), the others go on.  The fields nfields .. P - 1 are computed from zeros and stored with the rest: they live in the workspace
// only.  `done_all` is written by the reduce kernel's one writer and read at the head of every kernel.

constexpr int KRYLOV_MANY_FIELDS = 8;

struct KrylovManyHead {                 // wlsqm/hip.py reads it as 8 x (8 doubles, 4 int32, 6 doubles) and one int32
    KrylovScalars f[KRYLOV_MANY_FIELDS];
    int done_all;
    int pad[31];                        // 128 bytes: what follows stays 16-byte aligned, as the 16-byte loads need
};
constexpr long long KRYLOV_MANY_HEAD = sizeof(KrylovManyHead) / sizeof(double);
constexpr int KRYLOV_MANY_VECTORS = 8;  // r, r0, p, v, s, t, phat, shat at the pitch; dinv is one double per point behind them

__host__ __device__ static inline int krylov_pitch(int nfields) { return nfields <= 2 ? 2 : nfields <= 4 ? 4 : 8; }
__host__ __device__ static inline long long krylov_many_partials(long long nwg, int pitch) { return (2 * pitch * nwg + 7) / 8 * 8; }

struct KrylovManyWork {
    KrylovManyHead* head; double* partial; long long nwg;       // partial: planes [sum][field][workgroup], 2 P nwg doubles
    double *r, *r0, *p, *v, *s, *t, *phat, *shat, *dinv;
};

static KrylovManyWork krylov_many_work(void* workspace, long long nrows, int pitch, bool preconditioned) {
    KrylovManyWork w;
    double* base = static_cast<double*>(workspace);
    w.head = static_cast<KrylovManyHead*>(workspace);
    w.nwg = (nrows + 255) / 256;
    w.partial = base + KRYLOV_MANY_HEAD;
    double* vec = w.partial + krylov_many_partials(w.nwg, pitch);
    const long long n = nrows * pitch;
    w.r = vec; w.r0 = vec + n; w.p = vec + 2 * n; w.v = vec + 3 * n; w.s = vec + 4 * n; w.t = vec + 5 * n;
    w.phat = preconditioned ? vec + 6 * n : w.p; w.shat = preconditioned ? vec + 7 * n : w.s;
    w.dinv = vec + 8 * n;
    return w;
}

struct KrylovFields {                   // a caller's (nfields, npoints) array: element (field, point) at at[field * sf + point * sp]
    double* at; long long sf, sp;
};

typedef double krylov_pair __attribute__((ext_vector_type(2)));

// The P fields of one point of an interleaved vector: 16-byte loads and stores (`at` is 16-byte aligned).
template <int P>
__device__ __forceinline__ void krylov_load_fields(const double* at, double (&f)[P]) {
#pragma unroll
    for (int q = 0; q < P; q += 2) {
        const krylov_pair two = *reinterpret_cast<const krylov_pair*>(at + q);
        f[q] = two.x; f[q + 1] = two.y;
    }
}

template <int P>
__device__ __forceinline__ void krylov_store_fields(double* at, const double (&f)[P], unsigned frozen) {
    if (frozen == 0) {                                           // uniform
#pragma unroll
        for (int q = 0; q < P; q += 2) {
            krylov_pair two;
            two.x = f[q]; two.y = f[q + 1];
            *reinterpret_cast<krylov_pair*>(at + q) = two;
        }
    } else {
#pragma unroll
        for (int q = 0; q < P; ++q)
            if (!((frozen >> q) & 1u)) at[q] = f[q];
    }
}

// Bit q: field q of the solve has stopped, and nothing of it may be written any more.
template <int P>
__device__ __forceinline__ unsigned krylov_frozen(const KrylovManyHead* head, int nfields) {
    unsigned frozen = 0;
#pragma unroll
    for (int q = 0; q < P; ++q)
        if (q < nfields && head->f[q].done) frozen |= 1u << q;
    return frozen;
}

template <int P> struct KrylovPacked {                           // the workspace's layout
    const double* at;
    __device__ __forceinline__ void load(long long point, double (&f)[P]) const { krylov_load_fields<P>(at + point * P, f); }
};

template <int P> struct KrylovStrided {                          // the caller's; the fields beyond nfields read as zeros
    const double* at; long long sf, sp; int nfields;
    __device__ __forceinline__ void load(long long point, double (&f)[P]) const {
#pragma unroll
        for (int q = 0; q < P; ++q) f[q] = q < nfields ? at[q * sf + point * sp] : 0.0;
    }
};

// krylov_row_sum for P fields: col and val are loaded once per entry, each field's sum is its own fma chain in entry order.
template <int P, class In>
__device__ __forceinline__ void krylov_row_sums(const int32_t* col, const double* val, const In& x, int wid, int n, double (&acc)[P]) {
    constexpr int UNROLL = 16 / P;                               // 128 bytes of x in flight per lane and batch, whatever the pitch
#pragma unroll
    for (int q = 0; q < P; ++q) acc[q] = 0.0;
    for (int e = 0; e < wid; e += UNROLL) {                      // wave-uniform
        if (e + UNROLL <= n) {
            double xs[UNROLL][P], vs[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const long long c = col[64LL * (e + u)];
                x.load(c, xs[u]);
                vs[u] = val[64LL * (e + u)];
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
#pragma unroll
                for (int q = 0; q < P; ++q) acc[q] = __builtin_fma(vs[u], xs[u][q], acc[q]);
        } else {
            for (int u = 0; u < UNROLL && e + u < n; ++u) {
                const long long c = col[64LL * (e + u)];
                const double v = val[64LL * (e + u)];
                double xs[P];
                x.load(c, xs);
#pragma unroll
                for (int q = 0; q < P; ++q) acc[q] = __builtin_fma(v, xs[q], acc[q]);
            }
        }
    }
}

// block_sums per field: partial[(plane * P + field) * nwg + blockIdx.x], each sum by block_sums' tree and wave order.
template <int P, bool TWO>
__device__ __forceinline__ void block_sums_many(double (&a)[P], double (&b)[P], double* partial, long long nwg) {
    __shared__ double part[2][P][4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int q = 0; q < P; ++q) {
            a[q] += __shfl_down(a[q], off, 64);
            if (TWO) b[q] += __shfl_down(b[q], off, 64);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < P; ++q) { part[0][q][wave] = a[q]; if (TWO) part[1][q][wave] = b[q]; }
    }
    __syncthreads();
    if (threadIdx.x < (TWO ? 2 : 1) * P) {
        const int plane = threadIdx.x / P, q = threadIdx.x % P;
        const double* w = part[plane][q];
        partial[(plane * P + q) * nwg + blockIdx.x] = ((w[0] + w[1]) + w[2]) + w[3];
    }
}

enum { SPMV_MANY_START = 0, SPMV_MANY_V = 1, SPMV_MANY_T = 2, SPMV_MANY_PRODUCT = 3 };

// krylov_spmv_kernel for P fields, y_q = M in_q:
//   START:   in = x and w = b the caller's; out = out2 = b - y interleaved, partials (out, out) and (b, b)
//   V:       all interleaved; out = y, partial (w, out)
//   T:       all interleaved; out = y, partials (out, w) and (out, out)
//   PRODUCT: T on the caller's in, w and out, whatever the state of a solve
template <int P, int MODE>
__global__ void __launch_bounds__(256) krylov_spmv_many_kernel(const KrylovSys m, int nfields, const KrylovFields in, const KrylovFields w,
                                                               const KrylovFields out, double* out2, double* partial,
                                                               const KrylovManyHead* head) {
    constexpr bool CALLERS_IN = MODE == SPMV_MANY_START || MODE == SPMV_MANY_PRODUCT;
    if (MODE != SPMV_MANY_PRODUCT && head->done_all) return;     // uniform: the whole grid
    const unsigned frozen = MODE == SPMV_MANY_PRODUCT ? 0u : krylov_frozen<P>(head, nfields);
    const int lane = threadIdx.x & 63;
    const long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long row = s * 64 + lane;
    double a[P], b[P];
#pragma unroll
    for (int q = 0; q < P; ++q) a[q] = b[q] = 0.0;
    if (s * 64 < m.nrows) {                                      // wave-uniform
        const int wid = __builtin_amdgcn_readfirstlane(m.width[s]);
        const long long at = m.soff[s] + lane;
        int n = row < m.nrows ? m.len[row] : 0;
        n = n < wid ? n : wid;
        double sum[P], xi[P], wi[P], y[P];
        const KrylovStrided<P> xin{in.at, in.sf, in.sp, nfields}, win{w.at, w.sf, w.sp, nfields};
        const KrylovPacked<P> xpk{in.at}, wpk{w.at};
        if (CALLERS_IN) krylov_row_sums<P>(m.col + at, m.val + at, xin, wid, n, sum);
        else krylov_row_sums<P>(m.col + at, m.val + at, xpk, wid, n, sum);
        if (row < m.nrows) {
            const double d = m.dvec ? m.dvec[row] : m.dconst;
            if (CALLERS_IN) { xin.load(row, xi); win.load(row, wi); }
            else { xpk.load(row, xi); wpk.load(row, wi); }
#pragma unroll
            for (int q = 0; q < P; ++q) y[q] = __builtin_fma(m.c, sum[q], d * xi[q]);
            if (MODE == SPMV_MANY_START) {
#pragma unroll
                for (int q = 0; q < P; ++q) {
                    y[q] = wi[q] - y[q];
                    a[q] = y[q] * y[q]; b[q] = wi[q] * wi[q];
                }
                krylov_store_fields<P>(out.at + row * P, y, frozen);
                krylov_store_fields<P>(out2 + row * P, y, frozen);
            } else {
#pragma unroll
                for (int q = 0; q < P; ++q) {
                    a[q] = wi[q] * y[q];
                    if (MODE != SPMV_MANY_V) b[q] = y[q] * y[q];
                }
                if (MODE == SPMV_MANY_PRODUCT) {
#pragma unroll
                    for (int q = 0; q < P; ++q)
                        if (q < nfields) out.at[q * out.sf + row * out.sp] = y[q];
                } else {
                    krylov_store_fields<P>(out.at + row * P, y, frozen);
                }
            }
        }
    }
    block_sums_many<P, MODE != SPMV_MANY_V>(a, b, partial, gridDim.x);
}

// p_q = r_q + beta_q (p_q - omega_q v_q) (a field's first iteration: p_q = r_q), with the field's own scalars.
template <int P>
__device__ __forceinline__ void krylov_next_p(const KrylovManyWork& k, long long i, double (&p)[P]) {
    double r[P], po[P], v[P];
    krylov_load_fields<P>(k.r + i * P, r);
    krylov_load_fields<P>(k.p + i * P, po);
    krylov_load_fields<P>(k.v + i * P, v);
#pragma unroll
    for (int q = 0; q < P; ++q) {
        const KrylovScalars* sc = &k.head->f[q];
        p[q] = r[q];
        if (sc->iterations > 0) {                                // uniform
            const double omega = sc->omega, beta = (sc->rho / sc->rho_old) * (sc->alpha / omega);
            p[q] = r[q] + beta * (po[q] - omega * v[q]);
        }
    }
}

// s_q = r_q - alpha_q v_q
template <int P>
__device__ __forceinline__ void krylov_next_s(const KrylovManyWork& k, long long i, double (&s)[P]) {
    double r[P], v[P];
    krylov_load_fields<P>(k.r + i * P, r);
    krylov_load_fields<P>(k.v + i * P, v);
#pragma unroll
    for (int q = 0; q < P; ++q) s[q] = r[q] - k.head->f[q].alpha * v[q];
}

// krylov_update_kernel for P fields; dinv (nullable: phat is p and shat is s) is the matrix's and serves every field.
template <int P, int MODE>
__global__ void __launch_bounds__(256) krylov_update_many_kernel(long long nrows, const KrylovManyWork k, const double* dinv, int nfields,
                                                                 const KrylovFields x) {
    if (k.head->done_all) return;                                // uniform: the whole grid
    const unsigned frozen = krylov_frozen<P>(k.head, nfields);
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (MODE != UPDATE_X) {
        if (i >= nrows) return;
        double u[P];
        if (MODE == UPDATE_P) krylov_next_p<P>(k, i, u);
        else krylov_next_s<P>(k, i, u);
        krylov_store_fields<P>((MODE == UPDATE_P ? k.p : k.s) + i * P, u, frozen);
        if (dinv) {
            const double di = dinv[i];
#pragma unroll
            for (int q = 0; q < P; ++q) u[q] = di * u[q];
            krylov_store_fields<P>((MODE == UPDATE_P ? k.phat : k.shat) + i * P, u, frozen);
        }
    } else {
        double a[P], b[P];
#pragma unroll
        for (int q = 0; q < P; ++q) a[q] = b[q] = 0.0;
        if (i < nrows) {
            double ph[P], sh[P], s[P], t[P], r0[P], r[P];
            krylov_load_fields<P>(k.phat + i * P, ph);
            krylov_load_fields<P>(k.shat + i * P, sh);
            krylov_load_fields<P>(k.s + i * P, s);
            krylov_load_fields<P>(k.t + i * P, t);
            krylov_load_fields<P>(k.r0 + i * P, r0);
#pragma unroll
            for (int q = 0; q < P; ++q) {
                const double alpha = k.head->f[q].alpha, omega = k.head->f[q].omega;
                if (q < nfields && !((frozen >> q) & 1u)) {      // uniform
                    double* xq = x.at + q * x.sf + i * x.sp;
                    *xq = *xq + (alpha * ph[q] + omega * sh[q]);
                }
                r[q] = s[q] - omega * t[q];
                a[q] = r0[q] * r[q]; b[q] = r[q] * r[q];
            }
            krylov_store_fields<P>(k.r + i * P, r, frozen);
        }
        block_sums_many<P, true>(a, b, k.partial, gridDim.x);
    }
}

// krylov_update_block_kernel for P fields: a column of W is loaded once and applied to every field, each field's p_(first + j) by its
// own cross-lane move.
template <int NB, int P, int MODE>
__global__ void __launch_bounds__(256) krylov_update_block_many_kernel(long long nrows, const KrylovManyWork k, const double* W, int nfields) {
    if (k.head->done_all) return;                                // uniform: the whole grid
    const unsigned frozen = krylov_frozen<P>(k.head, nfields);
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, b0 = lane & ~(NB - 1);
    const long long s = i >> 6;
    if (s * 64 >= nrows) return;                                 // wave-uniform
    const bool live = i < nrows;
    double u[P], z[P];
#pragma unroll
    for (int q = 0; q < P; ++q) u[q] = z[q] = 0.0;
    if (live) {
        if (MODE == UPDATE_P) krylov_next_p<P>(k, i, u);
        else krylov_next_s<P>(k, i, u);
        krylov_store_fields<P>((MODE == UPDATE_P ? k.p : k.s) + i * P, u, frozen);
    }
    const double* w = W + (s * NB) * 64 + lane;
#pragma unroll 4                                                 // four columns of W in flight: unrolled further, P = 8 runs out of registers
    for (int j = 0; j < NB; ++j) {
        const double wj = w[64LL * j];
#pragma unroll
        for (int q = 0; q < P; ++q) z[q] = __builtin_fma(wj, __shfl(u[q], b0 + j, 64), z[q]);
    }
    if (live) krylov_store_fields<P>((MODE == UPDATE_P ? k.phat : k.shat) + i * P, z, frozen);
}

// krylov_reduce_kernel for P fields: one workgroup, each field's partials in krylov_reduce_kernel's order, then one lane runs the scalar
// step field after field and writes done_all.  REDUCE_DIAG: `partial` is one plane of counts, which belongs to the matrix and so to every
// field; the heads beyond nfields are set to a solve that has stopped.
template <int P>
__global__ void __launch_bounds__(256) krylov_reduce_many_kernel(int mode, const double* partial, long long nwg, int planes,
                                                                 KrylovManyHead* head, int nfields, double rtol, double atol, int maxiter) {
    const bool iterating = mode != REDUCE_DIAG && mode != REDUCE_PRODUCT;
    if (iterating && head->done_all) return;                     // uniform
    __shared__ double part[2][P][4];
    // every field's sum is thread t's t, t + 256, ... in that order; the loads of four such steps of all fields are in flight together
    // (field after field, one load at a time, this kernel took eight times the single-field one's time at P = 8)
    constexpr int STEPS = 4;
    double a[P], b[P];
    bool take[P];
#pragma unroll
    for (int q = 0; q < P; ++q) {
        a[q] = b[q] = 0.0;
        take[q] = mode == REDUCE_DIAG ? q == 0 : q < nfields && !(iterating && head->f[q].done);              // uniform
    }
    for (long long i0 = threadIdx.x; i0 < nwg; i0 += 256 * STEPS) {
        double va[STEPS][P], vb[STEPS][P];
#pragma unroll
        for (int u = 0; u < STEPS; ++u) {
            const long long i = i0 + 256 * u;
#pragma unroll
            for (int q = 0; q < P; ++q) {
                const bool on = take[q] && i < nwg;
                va[u][q] = on ? partial[q * nwg + i] : 0.0;
                vb[u][q] = on && planes > 1 ? partial[(P + q) * nwg + i] : 0.0;
            }
        }
#pragma unroll
        for (int u = 0; u < STEPS; ++u) {
            if (i0 + 256 * u < nwg) {
#pragma unroll
                for (int q = 0; q < P; ++q) {
                    if (take[q]) a[q] += va[u][q];
                    if (take[q] && planes > 1) b[q] += vb[u][q];
                }
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int q = 0; q < P; ++q) {
            a[q] += __shfl_down(a[q], off, 64);
            b[q] += __shfl_down(b[q], off, 64);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < P; ++q) { part[0][q][wave] = a[q]; part[1][q][wave] = b[q]; }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (mode == REDUCE_DIAG) {
        const double bad = ((part[0][0][0] + part[0][0][1]) + part[0][0][2]) + part[0][0][3];
        for (int q = 0; q < KRYLOV_MANY_FIELDS; ++q) {
            KrylovScalars* sc = &head->f[q];
            krylov_scalar_step(mode, sc, bad, 0.0, rtol, atol, maxiter);
            if (q >= nfields) { sc->rr = 0.0; krylov_stop(sc, KRYLOV_CONVERGED); }
        }
    } else {
#pragma unroll
        for (int q = 0; q < P; ++q) {
            if (q >= nfields || (iterating && head->f[q].done)) continue;
            const double s0 = ((part[0][q][0] + part[0][q][1]) + part[0][q][2]) + part[0][q][3];
            const double s1 = ((part[1][q][0] + part[1][q][1]) + part[1][q][2]) + part[1][q][3];
            krylov_scalar_step(mode, &head->f[q], s0, s1, rtol, atol, maxiter);
        }
    }
    if (mode == REDUCE_PRODUCT) return;
    int all = 1;
    for (int q = 0; q < nfields; ++q) all &= head->f[q].done ? 1 : 0;
    head->done_all = all;
}

static bool krylov_many_precond(int precond) { return precond == 0 || precond == 1 || precond == 8 || precond == 16 || precond == 32; }

static int krylov_many_arguments(const char* who, int64_t nrows, int64_t nslices, int nfields, int precond, const void* planes,
                                 const void* workspace) {
    if (reinterpret_cast<uintptr_t>(workspace) % 16) { set_error(std::string(who) + ": the workspace must be 16-byte aligned"); return WLSQM_EVALUE; }
    if (nfields < 1 || nfields > KRYLOV_MANY_FIELDS) { set_error(std::string(who) + ": nfields must be 1 .. 8"); return WLSQM_EVALUE; }
    if (!krylov_many_precond(precond)) { set_error(std::string(who) + ": precond must be 0, 1, 8, 16 or 32"); return WLSQM_EVALUE; }
    if (precond > 1) {
        if (!planes) { set_error(std::string(who) + ": null array"); return WLSQM_EVALUE; }
        if (nslices != (nrows + 63) / 64) { set_error(std::string(who) + ": nslices must be ceil(nrows / 64)"); return WLSQM_EVALUE; }
    }
    return WLSQM_OK;
}

template <int P>
static void krylov_many_reduce(int mode, const double* partial, long long nwg, int planes, const KrylovManyWork& w, int nfields, double rtol,
                               double atol, int maxiter, hipStream_t s) {
    hipLaunchKernelGGL(krylov_reduce_many_kernel<P>, dim3(1), dim3(256), 0, s, mode, partial, nwg, planes, w.head, nfields, rtol, atol, maxiter);
}

template <int P>
static void krylov_many_start(const KrylovSys& m, const KrylovManyWork& w, int nfields, const KrylovFields& b, const KrylovFields& x,
                              int precond, const void* planes, int64_t nslices, double rtol, double atol, int maxiter, hipStream_t s) {
    const dim3 grid((unsigned)w.nwg);
    if (precond == 1) {
        hipLaunchKernelGGL(krylov_diag_kernel, grid, dim3(256), 0, s, m, w.dinv, w.partial);
        note_kernel("krylov-diag");
    }
    const double* counts = precond > 1 ? static_cast<const double*>(planes) + krylov_plane_doubles(nslices, precond) : w.partial;
    krylov_many_reduce<P>(REDUCE_DIAG, counts, precond ? w.nwg : 0, 1, w, nfields, rtol, atol, maxiter, s);
    hipLaunchKernelGGL((krylov_spmv_many_kernel<P, SPMV_MANY_START>), grid, dim3(256), 0, s, m, nfields, x, b, KrylovFields{w.r, 0, 0}, w.r0,
                       w.partial, (const KrylovManyHead*)w.head);
    note_kernel("krylov-spmv-many");
    krylov_many_reduce<P>(REDUCE_RESIDUAL, w.partial, w.nwg, 2, w, nfields, rtol, atol, maxiter, s);
    note_kernel("krylov-reduce-many");
}

// NB 0: the Jacobi diagonal (w.dinv) or, with dinv null, no preconditioner.
template <int P, int NB>
static void krylov_many_iterations(const KrylovSys& m, const KrylovManyWork& w, int nfields, const KrylovFields& x, const double* dinv,
                                   const double* W, int64_t niter, hipStream_t s) {
    const dim3 grid((unsigned)w.nwg), block(256);
    const KrylovManyHead* head = w.head;
    const long long nrows = m.nrows;
    const KrylovFields none{nullptr, 0, 0};
    for (int64_t it = 0; it < niter; ++it) {
        if constexpr (NB > 0) hipLaunchKernelGGL((krylov_update_block_many_kernel<NB, P, UPDATE_P>), grid, block, 0, s, nrows, w, W, nfields);
        else hipLaunchKernelGGL((krylov_update_many_kernel<P, UPDATE_P>), grid, block, 0, s, nrows, w, dinv, nfields, none);
        hipLaunchKernelGGL((krylov_spmv_many_kernel<P, SPMV_MANY_V>), grid, block, 0, s, m, nfields, KrylovFields{w.phat, 0, 0},
                           KrylovFields{w.r0, 0, 0}, KrylovFields{w.v, 0, 0}, (double*)nullptr, w.partial, head);
        krylov_many_reduce<P>(REDUCE_ALPHA, w.partial, w.nwg, 1, w, nfields, 0.0, 0.0, 0, s);
        if constexpr (NB > 0) hipLaunchKernelGGL((krylov_update_block_many_kernel<NB, P, UPDATE_S>), grid, block, 0, s, nrows, w, W, nfields);
        else hipLaunchKernelGGL((krylov_update_many_kernel<P, UPDATE_S>), grid, block, 0, s, nrows, w, dinv, nfields, none);
        hipLaunchKernelGGL((krylov_spmv_many_kernel<P, SPMV_MANY_T>), grid, block, 0, s, m, nfields, KrylovFields{w.shat, 0, 0},
                           KrylovFields{w.s, 0, 0}, KrylovFields{w.t, 0, 0}, (double*)nullptr, w.partial, head);
        krylov_many_reduce<P>(REDUCE_OMEGA, w.partial, w.nwg, 2, w, nfields, 0.0, 0.0, 0, s);
        hipLaunchKernelGGL((krylov_update_many_kernel<P, UPDATE_X>), grid, block, 0, s, nrows, w, dinv, nfields, x);
        krylov_many_reduce<P>(REDUCE_RHO, w.partial, w.nwg, 2, w, nfields, 0.0, 0.0, 0, s);
    }
}

template <int P>
static void krylov_many_iterate(const KrylovSys& m, const KrylovManyWork& w, int nfields, const KrylovFields& x, int precond, const void* planes,
                                int64_t niter, hipStream_t s) {
    const double* W = static_cast<const double*>(planes);
    switch (precond) {
    case 8: krylov_many_iterations<P, 8>(m, w, nfields, x, nullptr, W, niter, s); break;
    case 16: krylov_many_iterations<P, 16>(m, w, nfields, x, nullptr, W, niter, s); break;
    case 32: krylov_many_iterations<P, 32>(m, w, nfields, x, nullptr, W, niter, s); break;
    default: krylov_many_iterations<P, 0>(m, w, nfields, x, precond ? w.dinv : nullptr, nullptr, niter, s); break;
    }
}

template <int P>
static void krylov_many_product(const KrylovSys& m, const KrylovManyWork& k, int nfields, const KrylovFields& in, const KrylovFields& w,
                                const KrylovFields& out, hipStream_t s) {
    hipLaunchKernelGGL((krylov_spmv_many_kernel<P, SPMV_MANY_PRODUCT>), dim3((unsigned)k.nwg), dim3(256), 0, s, m, nfields, in, w, out,
                       (double*)nullptr, k.partial, (const KrylovManyHead*)k.head);
    krylov_many_reduce<P>(REDUCE_PRODUCT, k.partial, k.nwg, 2, k, nfields, 0.0, 0.0, 0, s);
}

// ---- BiCGSTAB(2): two BiCG steps, then one residual minimisation over span(A r, A^2 r), A = M P ---------------
// A cycle is 14 launches, 4 products and 5 reduce steps, and counts as 2 iterations:
//   U0  u = r - beta u (the first cycle: u = r), hat = P u              P1  u1 = M hat, (rt, u1)             R  alpha
//   U1  r -= alpha u1, dy = alpha u, hat = P r                          P2  r1 = M hat, (rt, r1)             R  beta
//   U2  u = r - beta u, u1 = r1 - beta u1, hat = P u1                   P3  u2 = M hat, (rt, u2)             R  alpha
//   U3  r -= alpha u1, r1 -= alpha u2, dy += alpha u, hat = P r1,       P4  r2 = M hat, (r2, r1), (r2, r2),  R  g1, g2, omega
//       (r1, r1), (r, r1)                                                   (r, r2)
//   U4  x += P (dy + g1 r + g2 r1), r = r - g1 r1 - g2 r2, u = u - g1 u1 - g2 u2, (rt, r), (r, r)            R  the stop, the next beta
// P1 .. P3 are krylov_spmv_kernel<SPMV_V>.  x is written by U4 alone, behind every check of the cycle's scalars.  Without a preconditioner
// hat is not stored and the products read u, r, u1, r1 themselves.  The scalars are KrylovScalars': rho the last (rt, r), rho_old the
// recurrence's rho0, and beta, g1, g2 in pad[0 .. 2].  The partials are 5 planes of nwg: U3 writes planes 0 and 1, P4 planes 2 .. 4.

constexpr int KRYLOV_L2_VECTORS = 10;   // r, r1, r2, u, u1, u2, rt, dy, hat, dinv
constexpr int KRYLOV_L2_PLANES = 5;

struct KrylovL2Work {
    KrylovScalars* sc; double* partial; long long nwg;
    double *r, *r1, *r2, *u, *u1, *u2, *rt, *dy, *hat, *dinv;   // hat null: no preconditioner; dinv null: none, or blocks
};

static KrylovL2Work krylov_l2_work(void* workspace, long long nrows, int precond) {
    KrylovL2Work w;
    double* base = static_cast<double*>(workspace);
    w.sc = static_cast<KrylovScalars*>(workspace);
    w.nwg = (nrows + 255) / 256;
    w.partial = base + KRYLOV_HEAD;
    double* vec = w.partial + KRYLOV_L2_PLANES * w.nwg;
    w.r = vec; w.r1 = vec + nrows; w.r2 = vec + 2 * nrows; w.u = vec + 3 * nrows; w.u1 = vec + 4 * nrows; w.u2 = vec + 5 * nrows;
    w.rt = vec + 6 * nrows; w.dy = vec + 7 * nrows;
    w.hat = precond ? vec + 8 * nrows : nullptr; w.dinv = precond == 1 ? vec + 9 * nrows : nullptr;
    return w;
}

// block_sums for three sums, into the planes 2 .. 4.
__device__ __forceinline__ void block_sums_three(double (&a)[3], double* partial, long long nwg) {
    __shared__ double part[3][4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int q = 0; q < 3; ++q) a[q] += __shfl_down(a[q], off, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 3; ++q) part[q][wave] = a[q];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const double* w = part[threadIdx.x];
        partial[(2 + threadIdx.x) * nwg + blockIdx.x] = ((w[0] + w[1]) + w[2]) + w[3];
    }
}

// P4: r2 = M in, with the partials (r2, r1), (r2, r2) and (r, r2).
__global__ void __launch_bounds__(256) krylov_l2_spmv_kernel(const KrylovSys m, const double* in, const double* r, const double* r1,
                                                             double* r2, double* partial, const KrylovScalars* sc) {
    if (sc->done) return;                                        // uniform: the whole grid
    const int lane = threadIdx.x & 63;
    const long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long row = s * 64 + lane;
    double a[3] = {0.0, 0.0, 0.0};
    if (s * 64 < m.nrows) {                                      // wave-uniform
        const int wid = __builtin_amdgcn_readfirstlane(m.width[s]);
        const long long at = m.soff[s] + lane;
        int n = row < m.nrows ? m.len[row] : 0;
        n = n < wid ? n : wid;
        const double sum = krylov_row_sum(m.col + at, m.val + at, in, wid, n);
        if (row < m.nrows) {
            const double d = m.dvec ? m.dvec[row] : m.dconst;
            const double y = __builtin_fma(m.c, sum, d * in[row]);
            r2[row] = y;
            a[0] = y * r1[row]; a[1] = y * y; a[2] = r[row] * y;
        }
    }
    block_sums_three(a, partial, gridDim.x);
}

// z = P v of this lane's row: the blocks' (every lane of the wave takes part, one beyond nrows with 0), the Jacobi diagonal's, or v.
template <int NB>
__device__ __forceinline__ double krylov_l2_precondition(const KrylovL2Work& k, const double* W, long long i, long long s, int lane,
                                                         bool live, double v) {
    if constexpr (NB > 0) return krylov_block_apply<NB>(W + (s * NB) * 64 + lane, live ? v : 0.0, lane);
    else return k.dinv && live ? k.dinv[i] * v : v;
}

enum { L2_U0 = 0, L2_U1 = 1, L2_U2 = 2, L2_U3 = 3, L2_U4 = 4 };

// The update STEP of the list above, with P the blocks of NB rows in W, or (NB 0) the Jacobi diagonal k.dinv or nothing.  DEFER: U4 leaves
// what P is to be applied to in k.hat and x alone (the approximate inverse adds P of it to x by a launch of its own, section 22).
template <int NB, int STEP, bool DEFER = false>
__global__ void __launch_bounds__(256) krylov_l2_update_kernel(long long nrows, const KrylovL2Work k, const double* W, double* x) {
    const KrylovScalars* sc = k.sc;
    if (sc->done) return;                                        // uniform: the whole grid
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const long long s = i >> 6;
    const bool live = i < nrows;
    double a = 0.0, b = 0.0;
    if (s * 64 < nrows) {                                        // wave-uniform
        double v = 0.0;                                          // what P is applied to
        if (live) {
            if (STEP == L2_U0) {
                v = k.r[i];
                if (sc->iterations > 0) v = v - sc->pad[0] * k.u[i];
                k.u[i] = v;
            } else if (STEP == L2_U1) {
                const double alpha = sc->alpha;
                v = k.r[i] - alpha * k.u1[i];
                k.r[i] = v;
                k.dy[i] = alpha * k.u[i];
            } else if (STEP == L2_U2) {
                const double beta = sc->pad[0];
                k.u[i] = k.r[i] - beta * k.u[i];
                v = k.r1[i] - beta * k.u1[i];
                k.u1[i] = v;
            } else if (STEP == L2_U3) {
                const double alpha = sc->alpha;
                const double r = k.r[i] - alpha * k.u1[i];
                v = k.r1[i] - alpha * k.u2[i];
                k.r[i] = r; k.r1[i] = v;
                k.dy[i] = k.dy[i] + alpha * k.u[i];
                a = v * v; b = r * v;
            } else {
                const double g1 = sc->pad[1], g2 = sc->pad[2];
                const double r = k.r[i], r1 = k.r1[i];
                v = (k.dy[i] + g1 * r) + g2 * r1;
                const double rn = (r - g1 * r1) - g2 * k.r2[i];
                k.r[i] = rn;
                k.u[i] = (k.u[i] - g1 * k.u1[i]) - g2 * k.u2[i];
                a = k.rt[i] * rn; b = rn * rn;
            }
        }
        const double z = krylov_l2_precondition<NB>(k, W, i, s, lane, live, v);
        if (live) {
            if (STEP == L2_U4 && !DEFER) x[i] = x[i] + z;
            else if (k.hat) k.hat[i] = z;
        }
    }
    if (STEP == L2_U3 || STEP == L2_U4) block_sums<true>(a, b, k.partial, gridDim.x);
}

enum { L2_START = 0, L2_ALPHA = 1, L2_BETA = 2, L2_ALPHA1 = 3, L2_MR = 4, L2_END = 5 };

// The head of the next cycle, taken where its (rt, r) is formed: rho0 = -omega rho0, beta = alpha rho1 / rho0, rho0 = rho1.
__device__ __forceinline__ void krylov_l2_next_cycle(KrylovScalars* sc, double rho1) {
    const double rho0 = -sc->omega * sc->rho_old;
    if (rho0 == 0.0) { krylov_stop(sc, KRYLOV_BREAKDOWN); return; }
    const double beta = sc->alpha * rho1 / rho0;
    if (!__builtin_isfinite(beta)) { krylov_stop(sc, KRYLOV_NONFINITE); return; }
    sc->pad[0] = beta; sc->rho_old = rho1;
}

// The scalar step of `mode` on the sums of its dot products: one lane.
__device__ __forceinline__ void krylov_l2_scalar_step(int mode, KrylovScalars* sc, const double (&s)[KRYLOV_L2_PLANES], double rtol, double atol) {
    switch (mode) {
    case L2_START: {                                             // s0 = (r, r) = (rt, r), s1 = (b, b), behind REDUCE_DIAG
        sc->rho = s[0]; sc->rr = s[0];
        if (!__builtin_isfinite(s[0]) || !__builtin_isfinite(s[1])) { krylov_stop(sc, KRYLOV_NONFINITE); break; }
        const double rel = rtol * __builtin_sqrt(s[1]), stop = rel > atol ? rel : atol;
        sc->stop = stop;
        if (__builtin_sqrt(s[0]) <= stop) { krylov_stop(sc, KRYLOV_CONVERGED); break; }
        if (sc->maxiter <= 0) { krylov_stop(sc, KRYLOV_MAXITER); break; }
        sc->rho_old = 1.0; sc->alpha = 0.0; sc->omega = 1.0;
        sc->pad[0] = sc->pad[1] = sc->pad[2] = 0.0;
        krylov_l2_next_cycle(sc, s[0]);
        break;
    }
    case L2_ALPHA:                                               // s0 = (rt, u1)
    case L2_ALPHA1: {                                            // s0 = (rt, u2)
        if (!__builtin_isfinite(s[0])) { krylov_stop(sc, KRYLOV_NONFINITE); break; }
        if (s[0] == 0.0) {
            if (mode == L2_ALPHA) { krylov_stop(sc, KRYLOV_BREAKDOWN); break; }
            // j = 1: the cycle already holds the step j = 0, which x has not received.  The breakdown waits for the cycle's end: alpha = 0
            // and rho0 = 0, so that x takes alpha_0 u_0 and the minimisation, and the next cycle's head answers 2 unless that converged
            // (a system of one row always ends here: its Krylov space has one dimension)
            sc->alpha = 0.0; sc->rho_old = 0.0;
            break;
        }
        const double alpha = sc->rho_old / s[0];
        if (!__builtin_isfinite(alpha)) { krylov_stop(sc, KRYLOV_NONFINITE); break; }
        sc->alpha = alpha;
        break;
    }
    case L2_BETA: {                                              // s0 = (rt, r1)
        if (!__builtin_isfinite(s[0])) { krylov_stop(sc, KRYLOV_NONFINITE); break; }
        if (sc->rho_old == 0.0) { krylov_stop(sc, KRYLOV_BREAKDOWN); break; }
        const double beta = sc->alpha * s[0] / sc->rho_old;
        if (!__builtin_isfinite(beta)) { krylov_stop(sc, KRYLOV_NONFINITE); break; }
        sc->pad[0] = beta; sc->rho_old = s[0];
        break;
    }
    case L2_MR: {                                                // s1 = (r1, r1), c1 = (r, r1), a12 = (r2, r1), a22 = (r2, r2), c2 = (r, r2)
        const double s1 = s[0], c1 = s[1], a12 = s[2], a22 = s[3], c2 = s[4];
        if (!__builtin_isfinite(s1) || !__builtin_isfinite(c1) || !__builtin_isfinite(a12) || !__builtin_isfinite(a22) || !__builtin_isfinite(c2)) {
            krylov_stop(sc, KRYLOV_NONFINITE);
            break;
        }
        double g1 = 0.0, g2 = 0.0;
        if (s1 != 0.0) {
            const double tau = a12 / s1, s2 = a22 - tau * a12;
            if (s2 != 0.0) g2 = (c2 - tau * c1) / s2;
            g1 = c1 / s1 - tau * g2;
        }
        if (!__builtin_isfinite(g1) || !__builtin_isfinite(g2)) { krylov_stop(sc, KRYLOV_NONFINITE); break; }
        sc->pad[1] = g1; sc->pad[2] = g2; sc->omega = g2;
        break;
    }
    default: {                                                   // L2_END: s0 = (rt, r), s1 = (r, r)
        const int it = sc->iterations + 2;
        sc->iterations = it; sc->rho = s[0]; sc->rr = s[1];
        if (!__builtin_isfinite(s[0]) || !__builtin_isfinite(s[1])) krylov_stop(sc, KRYLOV_NONFINITE);
        else if (__builtin_sqrt(s[1]) <= sc->stop) krylov_stop(sc, KRYLOV_CONVERGED);
        else if (it >= sc->maxiter) krylov_stop(sc, KRYLOV_MAXITER);
        else krylov_l2_next_cycle(sc, s[0]);
        break;
    }
    }
}

// krylov_reduce_kernel for up to five planes: thread t sums t, t + 256, ... of each, then the tree, the waves in order and one lane's step.
__global__ void __launch_bounds__(256) krylov_l2_reduce_kernel(int mode, const double* partial, long long nwg, KrylovScalars* sc,
                                                               double rtol, double atol) {
    if (sc->done) return;                                        // uniform
    const int planes = mode == L2_MR ? 5 : (mode == L2_START || mode == L2_END) ? 2 : 1;
    __shared__ double part[KRYLOV_L2_PLANES][4];
    double a[KRYLOV_L2_PLANES];
#pragma unroll
    for (int q = 0; q < KRYLOV_L2_PLANES; ++q) a[q] = 0.0;
    for (long long i = threadIdx.x; i < nwg; i += 256) {
#pragma unroll
        for (int q = 0; q < KRYLOV_L2_PLANES; ++q)
            if (q < planes) a[q] += partial[q * nwg + i];        // uniform
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int q = 0; q < KRYLOV_L2_PLANES; ++q) a[q] += __shfl_down(a[q], off, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < KRYLOV_L2_PLANES; ++q) part[q][wave] = a[q];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sums[KRYLOV_L2_PLANES];
#pragma unroll
    for (int q = 0; q < KRYLOV_L2_PLANES; ++q) sums[q] = ((part[q][0] + part[q][1]) + part[q][2]) + part[q][3];
    krylov_l2_scalar_step(mode, sc, sums, rtol, atol);
}

template <int NB>
static void krylov_l2_cycles(const KrylovSys& m, const KrylovL2Work& w, const double* W, double* x, int64_t ncycles, hipStream_t s) {
    const dim3 grid((unsigned)w.nwg), block(256);
    const KrylovScalars* sc = w.sc;
    const long long nrows = m.nrows;
    const double* rt = w.rt;
    const double *in_u = w.hat ? w.hat : w.u, *in_r = w.hat ? w.hat : w.r, *in_u1 = w.hat ? w.hat : w.u1, *in_r1 = w.hat ? w.hat : w.r1;
    double* const none = nullptr;
    auto reduce = [&](int mode) {
        hipLaunchKernelGGL(krylov_l2_reduce_kernel, dim3(1), block, 0, s, mode, (const double*)w.partial, w.nwg, w.sc, 0.0, 0.0);
    };
    for (int64_t it = 0; it < ncycles; ++it) {
        hipLaunchKernelGGL((krylov_l2_update_kernel<NB, L2_U0>), grid, block, 0, s, nrows, w, W, none);
        hipLaunchKernelGGL((krylov_spmv_kernel<SPMV_V>), grid, block, 0, s, m, in_u, rt, w.u1, none, w.partial, sc, 0);
        reduce(L2_ALPHA);
        hipLaunchKernelGGL((krylov_l2_update_kernel<NB, L2_U1>), grid, block, 0, s, nrows, w, W, none);
        hipLaunchKernelGGL((krylov_spmv_kernel<SPMV_V>), grid, block, 0, s, m, in_r, rt, w.r1, none, w.partial, sc, 0);
        reduce(L2_BETA);
        hipLaunchKernelGGL((krylov_l2_update_kernel<NB, L2_U2>), grid, block, 0, s, nrows, w, W, none);
        hipLaunchKernelGGL((krylov_spmv_kernel<SPMV_V>), grid, block, 0, s, m, in_u1, rt, w.u2, none, w.partial, sc, 0);
        reduce(L2_ALPHA1);
        hipLaunchKernelGGL((krylov_l2_update_kernel<NB, L2_U3>), grid, block, 0, s, nrows, w, W, none);
        hipLaunchKernelGGL(krylov_l2_spmv_kernel, grid, block, 0, s, m, in_r1, (const double*)w.r, (const double*)w.r1, w.r2, w.partial, sc);
        reduce(L2_MR);
        hipLaunchKernelGGL((krylov_l2_update_kernel<NB, L2_U4>), grid, block, 0, s, nrows, w, W, x);
        reduce(L2_END);
    }
}

// ---- the sparse approximate inverse: Q = diag(qd) + (plane qv on the matrix's own structure), Q M ~ I ----------
// Row i of Q minimises ||q^T M - e_i^T||_2 over the pattern of row i of M.  Its unknowns are the slots: slot 0 the diagonal (column i),
// slot k the stored entry k - 1 of row i; a slot whose column an earlier slot names is dead, its coefficient 0.0.  With J the columns of
// the slots and m_r row r of M (d_r at column r, then c val[r, e] at col[r, e]): G[a, b] = m_J[a] . m_J[b], rhs[a] = (m_J[a])_i, G q = rhs
// by LDL^T without pivoting.
// The planes: qd (nrows), the per-slice counts of the rows whose factorisation failed (ceil(nrows / 64)), qv (the matrix's `total`).
//
// An own entry (column r in row r) is part of the row's diagonal: every row is read as d_r plus its own entries in entry order, then its
// other entries.  A row may store 65 entries where the 65th is its own entry (64 neighbours of an F-known point); otherwise 64.
// krylov_spai_kernel: one wave per slice, its 64 rows one after the other; lane l owns slot l + 1 and keeps row J[l + 1] of M in registers.
//   columns: every column of the rows of J gets a cell of an LDS table by open addressing (atomicCAS on the key).  The cell numbers serve
//            matching only: no sum runs in their order.
//   row b, dense: its owner stores d at the cell of its diagonal and every entry at its cell; an entry whose column the row named before
//            (the own entry of an F-known row, a neighbour named twice) is added onto the cell afterwards, in entry order.
//   G[a, b], b <= a: lane a's fma chain over ITS entries as stored, the diagonal first, against the dense row b.  rhs[b] = dense b at i.
//   LDL^T in LDS, right-looking, lane a updating row a; the forward substitution rides on it; then the division and the backward pass.
// A pivot that is not positive and finite, a slot that names no row, or a non-finite coefficient counts the row as failed: its row of Q
// is zeros, and every start reduces the counts into status 4.  No atomics on anything that is summed, no scratch memory.

constexpr int KRYLOV_SPAI_CAP = 65;     // stored entries per row: 64, and behind them the row's own entry

__host__ __device__ constexpr int krylov_spai_cells(int W) { return ((W + 1) * (W + 1) * 9 / 8 + 63) / 64 * 64; }   // > 1 + W + W^2 columns

struct KrylovSpai {
    double *qd, *counts, *qv;
};

static KrylovSpai krylov_spai_planes(const void* planes, long long nrows) {
    double* base = static_cast<double*>(const_cast<void*>(planes));
    return KrylovSpai{base, base + nrows, base + nrows + (nrows + 63) / 64};
}

// The cell of column c: the first free one at or behind its hash, or the one that holds it already.
template <int CELLS>
__device__ __forceinline__ int krylov_spai_cell(int32_t* keys, int32_t c) {
    unsigned at = (unsigned)(((unsigned long long)((unsigned)c * 2654435761u) * (unsigned)CELLS) >> 32);
    for (;;) {
        const int32_t old = atomicCAS(&keys[at], -1, c);
        if (old == -1 || old == c) return (int)at;
        at = at + 1 == (unsigned)CELLS ? 0u : at + 1;
    }
}

template <int W>
__global__ void __launch_bounds__(64) krylov_spai_kernel(const KrylovSys m, double* qd, double* qv, double* counts) {
    constexpr int CELLS = krylov_spai_cells(W);
    __shared__ int32_t keys[CELLS];
    __shared__ unsigned long long cells[CELLS];                  // the dense row (a double's bits), and the marks of the rows that named a cell
    __shared__ double G[(W + 1) * (W + 2) / 2];                  // the lower triangle, row a at a (a + 1) / 2
    const int lane = threadIdx.x;
    const long long s = blockIdx.x;
    const long long first = s * 64, last = first + 64 < m.nrows ? first + 64 : m.nrows;
    const int wid = m.width[s];
    const long long soff = m.soff[s];
    const unsigned long long bit = 1ull << lane;
    auto dense = [&](int cell) { return __longlong_as_double((long long)cells[cell]); };
    auto put = [&](int cell, double v) { cells[cell] = (unsigned long long)__double_as_longlong(v); };
    int failed = 0;
    for (long long i = first; i < last; ++i) {                   // uniform
        int ni = m.len[i];
        ni = __builtin_amdgcn_readfirstlane(ni < wid ? ni : wid);
        const bool extra = W == 64 && ni > 64;                   // a 65th entry: the own entry behind 64 neighbours, or the row fails
        ni = ni < W ? ni : W;
        const long long at_i = soff + (i - first) + 64LL * lane;
        const bool mine = lane < ni;
        const long long r = mine ? (long long)m.col[at_i] : -1;
        double ti = mine ? m.c * m.val[at_i] : 0.0;
        double di = m.dvec ? m.dvec[i] : m.dconst;
        bool wild = mine && (r < 0 || r >= m.nrows);
        // own entries (column i) belong to the diagonal: added onto d_i in entry order, in every row
        for (unsigned long long left = __ballot(mine && r == i); left; left &= left - 1) di += __shfl(ti, __builtin_ctzll(left), 64);
        if (extra) {
            if (m.col[at_i - 64LL * lane + 64LL * 64] == i) di += m.c * m.val[at_i - 64LL * lane + 64LL * 64];
            else wild = true;
        }
        if (mine && r == i) ti = 0.0;
        bool dead = mine && r == i;
        for (int l = 0; l < ni; ++l) {                           // uniform
            const long long rl = __shfl(r, l, 64);
            if (l < lane && rl == r) dead = true;
        }
        const bool live = mine && !dead && !wild;
        const unsigned long long livemask = __ballot(live), deadmask = __ballot(mine && !live && !wild && r != i);
        for (int t = lane; t < CELLS; t += 64) { keys[t] = -1; cells[t] = 0ull; }
        const int a = lane + 1, row_a = a * (a + 1) / 2;
        if (mine)
            for (int b = 0; b <= a; ++b) G[row_a + b] = b == a && !live ? 1.0 : 0.0;     // a dead slot is an identity row
        __syncthreads();
        // the cells of the columns, and lane l's row J[l + 1] into its registers
        const int cell_i = krylov_spai_cell<CELLS>(keys, (int32_t)i);
        const int cell_d = mine && !wild ? krylov_spai_cell<CELLS>(keys, (int32_t)r) : cell_i;
        int n = 0;
        long long at_r = 0;
        double dr = 0.0;
        bool extra_r = false;
        if (live) {
            const int wr = m.width[r >> 6];
            n = m.len[r];
            n = n < wr ? n : wr;
            extra_r = W == 64 && n > 64;
            n = n < W ? n : W;
            at_r = m.soff[r >> 6] + (r & 63);
            dr = m.dvec ? m.dvec[r] : m.dconst;
        }
        int nmax = n;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(nmax, off, 64); nmax = o > nmax ? o : nmax; }
        nmax = __builtin_amdgcn_readfirstlane(nmax);
        double tv[W];
        int cell[W];
        unsigned long long use = 0ull;                           // bit e: entry e is a neighbour's (not an own entry, which dr takes)
#pragma unroll
        for (int e = 0; e < W; ++e) {
            tv[e] = 0.0; cell[e] = cell_i;
            if (e < nmax) {                                      // uniform
                if (e < n) {
                    const int32_t c = m.col[at_r + 64LL * e];
                    const double t = m.c * m.val[at_r + 64LL * e];
                    if (c == r) {
                        dr += t;
                    } else {
                        tv[e] = t;
                        cell[e] = krylov_spai_cell<CELLS>(keys, c);
                        use |= 1ull << e;
                    }
                }
            }
        }
        bool lost = false;
        if (extra_r) {
            if (m.col[at_r + 64LL * 64] == r) dr += m.c * m.val[at_r + 64LL * 64];
            else lost = true;
        }
        if (__ballot(lost) != 0ull) wild = true;                 // uniform from here: the row fails
        __syncthreads();
        // which of the lane's entries name a column that its row named before (the diagonal first): bit e of again
        unsigned long long again = 0ull;
        if (live) atomicOr(&cells[cell_d], bit);
#pragma unroll
        for (int e = 0; e < W; ++e)
            if (e < nmax && ((use >> e) & 1ull) && (atomicOr(&cells[cell[e]], bit) & bit)) again |= 1ull << e;
        __syncthreads();
        for (int t = lane; t < CELLS; t += 64) cells[t] = 0ull;
        __syncthreads();
        // slot 0, row i itself: d_i, the entries of the live slots, then those of the dead ones in entry order
        if (lane == 0) put(cell_i, di);
        __syncthreads();
        if (live) put(cell_d, ti);
        __syncthreads();
        for (unsigned long long left = deadmask; left; left &= left - 1) {        // uniform
            if (lane == __builtin_ctzll(left)) put(cell_d, dense(cell_d) + ti);
            __syncthreads();
        }
        const double rhs0 = dense(cell_i);
        {
            double acc = 0.0;
            if (live) {
                acc = __builtin_fma(dr, dense(cell_d), acc);
#pragma unroll
                for (int e = 0; e < W; ++e)
                    if (e < nmax) acc = __builtin_fma(tv[e], dense(cell[e]), acc);
                G[row_a] = acc;
            }
            const double xl = mine ? dense(cell_d) : 0.0;
            double g00 = __builtin_fma(di, rhs0, 0.0);
            for (int l = 0; l < ni; ++l) g00 = __builtin_fma(__shfl(ti, l, 64), __shfl(xl, l, 64), g00);
            if (lane == 0) G[0] = g00;
        }
        __syncthreads();
        if (mine) cells[cell_d] = 0ull;
        if (lane == 0) cells[cell_i] = 0ull;
        __syncthreads();
        // the live slots, one after the other: the owner spreads its row, every lane at or behind it forms its G[a, b]
        double rhs = 0.0;
        for (unsigned long long left = livemask; left; left &= left - 1) {        // uniform
            const int lb = __builtin_ctzll(left);
            if (lane == lb) {
                put(cell_d, dr);
#pragma unroll
                for (int e = 0; e < W; ++e)
                    if (e < nmax && ((use & ~again) >> e) & 1ull) put(cell[e], tv[e]);
#pragma unroll
                for (int e = 0; e < W; ++e)
                    if (e < nmax && ((again >> e) & 1ull)) put(cell[e], dense(cell[e]) + tv[e]);
                rhs = dense(cell_i);
            }
            __syncthreads();
            if (live && lane >= lb) {
                double acc = __builtin_fma(dr, dense(cell_d), 0.0);
#pragma unroll
                for (int e = 0; e < W; ++e)
                    if (e < nmax) acc = __builtin_fma(tv[e], dense(cell[e]), acc);
                G[row_a + lb + 1] = acc;
            }
            __syncthreads();
            if (lane == lb) {
                cells[cell_d] = 0ull;
#pragma unroll
                for (int e = 0; e < W; ++e)
                    if (e < nmax && ((use >> e) & 1ull)) cells[cell[e]] = 0ull;
            }
            __syncthreads();
        }
        // G = L D L^T in place, L y = rhs with it, then z = D^-1 y and L^T q = z
        bool bad = __ballot(wild) != 0ull;
        double y = rhs, y0 = rhs0;
        for (int k = 0; k <= ni && !bad; ++k) {                  // uniform
            const double dk = G[k * (k + 1) / 2 + k];
            if (!(dk > 0.0 && __builtin_isfinite(dk))) { bad = true; break; }
            const double yk = k == 0 ? y0 : __shfl(y, k - 1, 64);
            double lak = 0.0;
            if (mine && a > k) {
                lak = G[row_a + k] / dk;
                for (int b = k + 1; b <= a; ++b) G[row_a + b] = __builtin_fma(-lak, G[b * (b + 1) / 2 + k], G[row_a + b]);
                y = __builtin_fma(-lak, yk, y);
            }
            __syncthreads();
            if (mine && a > k) G[row_a + k] = lak;
            __syncthreads();
        }
        double q = 0.0, q0 = 0.0;
        if (!bad) {                                              // uniform
            q = mine ? y / G[row_a + a] : 0.0;
            q0 = y0 / G[0];
            for (int k = ni; k >= 1; --k) {                      // uniform: slot k is final, the slots before it take it off
                const double qk = __shfl(q, k - 1, 64);
                const int row_k = k * (k + 1) / 2;
                if (mine && a < k) q = __builtin_fma(-G[row_k + a], qk, q);
                q0 = __builtin_fma(-G[row_k], qk, q0);
            }
            if (__ballot(!__builtin_isfinite(q)) != 0ull || !__builtin_isfinite(q0)) bad = true;
        }
        if (lane == 0) qd[i] = bad ? 0.0 : q0;
        if (mine) qv[at_i] = bad || !live ? 0.0 : q;
        if (extra && lane == 0) qv[at_i + 64LL * 64] = 0.0;
        failed += bad ? 1 : 0;
        __syncthreads();
    }
    if (lane == 0) counts[s] = (double)failed;
}

// The transposed planes: qd and the counts as they are, qv through the operator's (dest, src) pairs into the transposed structure.
__global__ void __launch_bounds__(256) krylov_spai_transpose_kernel(long long npairs, const int32_t* dest, const int32_t* src, long long head,
                                                                    const double* planes, double* planes_t) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < head) planes_t[t] = planes[t];
    if (t < npairs) planes_t[head + dest[t]] = planes[head + src[t]];
}

// out = Q in, or (acc) acc += Q in: krylov_spmv_kernel's row sum on the plane qv with the diagonal qd and c = 1, no dot product.
__global__ void __launch_bounds__(256) krylov_spai_apply_kernel(const KrylovSys q, const double* in, double* out, double* acc,
                                                                const KrylovScalars* sc, int always) {
    if (!always && sc->done) return;                             // uniform: the whole grid
    const int lane = threadIdx.x & 63;
    const long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long row = s * 64 + lane;
    if (s * 64 >= q.nrows) return;                               // wave-uniform
    const int wid = __builtin_amdgcn_readfirstlane(q.width[s]);
    const long long at = q.soff[s] + lane;
    int n = row < q.nrows ? q.len[row] : 0;
    n = n < wid ? n : wid;
    const double sum = krylov_row_sum(q.col + at, q.val + at, in, wid, n);
    if (row < q.nrows) {
        const double z = __builtin_fma(q.c, sum, q.dvec[row] * in[row]);
        if (acc) acc[row] = acc[row] + z;
        else out[row] = z;
    }
}

static KrylovSys krylov_spai_system(const KrylovSys& m, const KrylovSpai& p) {
    KrylovSys q = m;
    q.val = p.qv; q.dvec = p.qd; q.dconst = 0.0; q.c = 1.0;
    return q;
}

static void krylov_spai_apply(const KrylovSys& q, long long nwg, const double* in, double* out, double* acc, const KrylovScalars* sc,
                              int always, hipStream_t s) {
    hipLaunchKernelGGL(krylov_spai_apply_kernel, dim3((unsigned)nwg), dim3(256), 0, s, q, in, out, acc, sc, always);
}

// An iteration of BiCGSTAB with a P that launches of its own apply (Q here, the overlapping blocks of section 28): krylov_update_kernel
// without a diagonal, then phat = P p and shat = P s by apply(in, out, acc): out = P in, or acc += P in.
template <class Apply>
static void krylov_applied_iterations(const KrylovSys& m, const Apply& apply, const KrylovWork& w, double* x, int64_t niter, hipStream_t s) {
    const dim3 grid((unsigned)w.nwg), block(256);
    const KrylovScalars* sc = w.sc;
    const long long nrows = m.nrows;
    double* const none = nullptr;
    for (int64_t it = 0; it < niter; ++it) {
        hipLaunchKernelGGL((krylov_update_kernel<UPDATE_P>), grid, block, 0, s, nrows, w, x, sc);
        apply((const double*)w.p, w.phat, none);
        hipLaunchKernelGGL((krylov_spmv_kernel<SPMV_V>), grid, block, 0, s, m, (const double*)w.phat, (const double*)w.r0, w.v, none, w.partial, sc, 0);
        krylov_reduce(REDUCE_ALPHA, w, w.nwg, 1, 0.0, 0.0, 0, s);
        hipLaunchKernelGGL((krylov_update_kernel<UPDATE_S>), grid, block, 0, s, nrows, w, x, sc);
        apply((const double*)w.s, w.shat, none);
        hipLaunchKernelGGL((krylov_spmv_kernel<SPMV_T>), grid, block, 0, s, m, (const double*)w.shat, (const double*)w.s, w.t, none, w.partial, sc, 0);
        krylov_reduce(REDUCE_OMEGA, w, w.nwg, 2, 0.0, 0.0, 0, s);
        hipLaunchKernelGGL((krylov_update_kernel<UPDATE_X>), grid, block, 0, s, nrows, w, x, sc);
        krylov_reduce(REDUCE_RHO, w, w.nwg, 2, 0.0, 0.0, 0, s);
    }
}

// A cycle of BiCGSTAB(2) with such a P, 19 launches: every update leaves what P is applied to in `pre` (the workspace's tenth vector), an
// apply forms hat = P pre for the product behind it, and the last one adds P pre to x: between U4, which every check of the cycle's
// scalars precedes, and the reduce that takes the stop.
template <class Apply>
static void krylov_applied_l2_cycles(const KrylovSys& m, const Apply& applied, const KrylovL2Work& w, double* pre, double* x, int64_t ncycles,
                                     hipStream_t s) {
    const dim3 grid((unsigned)w.nwg), block(256);
    const KrylovScalars* sc = w.sc;
    const long long nrows = m.nrows;
    const double *rt = w.rt, *hat = w.hat, *W = nullptr;
    double* const none = nullptr;
    KrylovL2Work u = w;                                          // the update kernels' view: their `hat` is pre, and no diagonal
    u.hat = pre; u.dinv = nullptr;
    auto reduce = [&](int mode) {
        hipLaunchKernelGGL(krylov_l2_reduce_kernel, dim3(1), block, 0, s, mode, (const double*)w.partial, w.nwg, w.sc, 0.0, 0.0);
    };
    auto apply = [&](double* acc) { applied((const double*)pre, w.hat, acc); };
    for (int64_t it = 0; it < ncycles; ++it) {
        hipLaunchKernelGGL((krylov_l2_update_kernel<0, L2_U0>), grid, block, 0, s, nrows, u, W, none);
        apply(none);
        hipLaunchKernelGGL((krylov_spmv_kernel<SPMV_V>), grid, block, 0, s, m, hat, rt, w.u1, none, w.partial, sc, 0);
        reduce(L2_ALPHA);
        hipLaunchKernelGGL((krylov_l2_update_kernel<0, L2_U1>), grid, block, 0, s, nrows, u, W, none);
        apply(none);
        hipLaunchKernelGGL((krylov_spmv_kernel<SPMV_V>), grid, block, 0, s, m, hat, rt, w.r1, none, w.partial, sc, 0);
        reduce(L2_BETA);
        hipLaunchKernelGGL((krylov_l2_update_kernel<0, L2_U2>), grid, block, 0, s, nrows, u, W, none);
        apply(none);
        hipLaunchKernelGGL((krylov_spmv_kernel<SPMV_V>), grid, block, 0, s, m, hat, rt, w.u2, none, w.partial, sc, 0);
        reduce(L2_ALPHA1);
        hipLaunchKernelGGL((krylov_l2_update_kernel<0, L2_U3>), grid, block, 0, s, nrows, u, W, none);
        apply(none);
        hipLaunchKernelGGL(krylov_l2_spmv_kernel, grid, block, 0, s, m, hat, (const double*)w.r, (const double*)w.r1, w.r2, w.partial, sc);
        reduce(L2_MR);
        hipLaunchKernelGGL((krylov_l2_update_kernel<0, L2_U4, true>), grid, block, 0, s, nrows, u, W, none);
        apply(x);
        reduce(L2_END);
    }
}

// The iterations (l2: the cycles) of a solve whose P is applied by launches of its own, on the method's own workspace.
template <class Apply>
static void krylov_applied_run(const KrylovSys& m, const Apply& apply, int l2, double* x, int64_t niter, void* workspace, hipStream_t s) {
    if (l2) {
        KrylovL2Work w = krylov_l2_work(workspace, m.nrows, 1);
        krylov_applied_l2_cycles(m, apply, w, w.dinv, x, niter, s);
    } else {
        KrylovWork w = krylov_work(workspace, m.nrows, true);
        w.dinv = nullptr;                                        // the update kernels form p and s only
        krylov_applied_iterations(m, apply, w, x, niter, s);
    }
}

// The start of such a solve: the `ncounts` counts of what the last build could not use into status 4, then the residual and its stop.
static int krylov_applied_start(const KrylovSys& m, const double* counts, long long ncounts, int l2, const double* b, const double* x,
                                double rtol, double atol, int64_t maxiter, void* workspace, hipStream_t s) {
    const long long nrows = m.nrows, nwg = (nrows + 255) / 256;
    const dim3 grid((unsigned)nwg);
    KrylovScalars* sc = static_cast<KrylovScalars*>(workspace);
    hipLaunchKernelGGL(krylov_reduce_kernel, dim3(1), dim3(256), 0, s, (int)REDUCE_DIAG, counts, ncounts, 1, sc, rtol, atol, (int)maxiter);
    if (l2) {
        const KrylovL2Work w = krylov_l2_work(workspace, nrows, 1);
        hipLaunchKernelGGL((krylov_spmv_kernel<SPMV_RESIDUAL>), grid, dim3(256), 0, s, m, x, b, w.r, w.rt, w.partial, (const KrylovScalars*)sc, 0);
        note_kernel("krylov-spmv-dot");
        hipLaunchKernelGGL(krylov_l2_reduce_kernel, dim3(1), dim3(256), 0, s, (int)L2_START, (const double*)w.partial, w.nwg, sc, rtol, atol);
        WLSQM_HIP_CHECK(hipGetLastError());
        note_kernel("krylov-l2-reduce");
        return WLSQM_OK;
    }
    const KrylovWork w = krylov_work(workspace, nrows, true);
    hipLaunchKernelGGL((krylov_spmv_kernel<SPMV_RESIDUAL>), grid, dim3(256), 0, s, m, x, b, w.r, w.r0, w.partial, (const KrylovScalars*)sc, 0);
    note_kernel("krylov-spmv-dot");
    krylov_reduce(REDUCE_RESIDUAL, w, w.nwg, 2, rtol, atol, (int)maxiter, s);
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("krylov-reduce");
    return WLSQM_OK;
}

static int krylov_spai_arguments(const char* who, int64_t nrows, int64_t nslices, const void* planes) {
    if (!planes) { set_error(std::string(who) + ": null array"); return WLSQM_EVALUE; }
    if (nslices != (nrows + 63) / 64) { set_error(std::string(who) + ": nslices must be ceil(nrows / 64)"); return WLSQM_EVALUE; }
    return WLSQM_OK;
}

static int krylov_tolerances(const char* who, const void* b, const void* x, double rtol, double atol, int64_t maxiter) {
    if (!b || !x) { set_error(std::string(who) + ": null array"); return WLSQM_EVALUE; }
    if (!(rtol >= 0.0) || !(atol >= 0.0) || !std::isfinite(rtol) || !std::isfinite(atol)) {
        set_error(std::string(who) + ": rtol and atol must be finite and >= 0");
        return WLSQM_EVALUE;
    }
    if (maxiter < 0 || maxiter > INT32_MAX) { set_error(std::string(who) + ": maxiter must be 0 .. 2^31 - 1"); return WLSQM_EVALUE; }
    return WLSQM_OK;
}

// ---- overlapping blocks: a restricted additive Schwarz preconditioner ------------------------------------------
// Block B is the rows B NB .. B NB + NB - 1, cut at nrows (cnt of them).  Its set ext_B is those rows followed by up to ROWS - cnt others,
// ascending, which the caller's table names (int32, (nblocks, ROWS), -1 where there are none; the block's own positions are taken from
// B, not from the table, and an entry that is no row, or one of the block's own, counts as -1; ascending order is the caller's to keep:
// a column is found by a binary search, and one that the search misses in an unsorted list is left out of A_B).  A_B = M[ext_B, ext_B], a -1 position an
// identity row and column, is inverted exactly and the first cnt rows of the inverse are kept: z[B NB + i] = sum_q W_B[i][q] v[ext_B[q]].
// The plane: W[(slice * ROWS + q) * 64 + lane] = entry (lane % NB, q) of W_B for the block that holds row slice * 64 + lane, so that a
// wave reads column q of its slice as one contiguous run of 512 bytes; zeros in the rows beyond nrows.  Behind the nslices * ROWS * 64
// doubles sit nslices * (64 / NB) more: per block position 1.0 where the last build could not invert, which every start reduces into
// status 4.  The transposed plane holds the first cnt rows of (A_B^T)^-1, the same preconditioner of M^T, from the same elimination.

struct KrylovSchwarz {
    int nb, rows;
    long long nblocks, nslots;          // the blocks of the matrix; the block positions of the plane, nslices * (64 / nb)
    double *W, *counts;
};

static KrylovSchwarz krylov_schwarz_planes(const void* planes, long long nrows, long long nslices, int nb, int rows) {
    double* base = static_cast<double*>(const_cast<void*>(planes));
    return KrylovSchwarz{nb, rows, (nrows + nb - 1) / nb, nslices * (64 / nb), base, base ? base + nslices * rows * 64 : nullptr};
}

// Position p of ext_B, or -1: `first` the block's first row, cnt its rows.
__device__ __forceinline__ long long krylov_schwarz_ext(const int32_t* table, long long B, int rows, int p, long long first, int cnt,
                                                        long long nrows) {
    if (p < cnt) return first + p;
    const long long r = table[B * rows + p];
    return r < 0 || r >= nrows || (r >= first && r < first + cnt) ? -1 : r;
}

// One wave per block, lane p the owner of row ext[p]: it looks its slice up by itself (the rows of a set lie in any slice), zeroes row p
// of the LDS image (ROWS x ROWS at the pitch ROWS + 1: a column is read without a bank conflict), and adds every stored entry whose
// column the set names onto (p, position), in entry order: the block's own columns by their range, the others by a binary search of the
// ascending rest of the list in LDS.  Then entry (p, q) = d delta_pq + c sum, as krylov_blocks_kernel forms it.
// The elimination is that kernel's, in place: Gauss-Jordan with partial pivoting, at step k the largest |entry k| among the rows that
// have not been a pivot, the lowest row at a tie, a NaN the largest; the pivot row times 1 / pivot goes through `prow` (with 1 / pivot
// in place k: column k of the image is a unit vector from here on, so it holds the column of the inverse that starts at this step), and
// every other lane eliminates its own row with fma.  Rows are not moved: entry (i, c) of the inverse ends at (who[i], step[c]), who[k]
// the pivot row of step k and step[r] the step of row r.  A zero or non-finite pivot or a non-finite entry counts the block as unusable.
template <int ROWS>
__global__ void __launch_bounds__(64) krylov_schwarz_build_kernel(const KrylovSys m, const KrylovSchwarz p, const int32_t* table, double* WT,
                                                                  double* counts_t) {
    constexpr int PITCH = ROWS + 1;
    __shared__ double a[ROWS * PITCH];
    __shared__ double prow[ROWS];
    __shared__ int32_t ext[ROWS], who_of[ROWS], step_of[ROWS];
    const int lane = threadIdx.x, nb = p.nb, bps = 64 / nb;
    const long long B = blockIdx.x, first = B * nb;
    const long long left = m.nrows - first;
    const int cnt = B >= p.nblocks || left <= 0 ? 0 : left < nb ? (int)left : nb;
    const int i_out = lane % nb, q_out = lane / nb;
    double* w = p.W + ((B / bps) * ROWS) * 64 + (B % bps) * nb + i_out;
    double* wt = WT ? WT + ((B / bps) * ROWS) * 64 + (B % bps) * nb + i_out : nullptr;
    if (cnt == 0) {                                              // uniform: a block position beyond the matrix
        for (int q = q_out; q < ROWS; q += bps) { w[64LL * q] = 0.0; if (wt) wt[64LL * q] = 0.0; }
        if (lane == 0) { p.counts[B] = 0.0; if (counts_t) counts_t[B] = 0.0; }
        return;
    }
    const bool owner = lane < ROWS;
    const long long r = owner ? krylov_schwarz_ext(table, B, ROWS, lane, first, cnt, m.nrows) : -1;
    if (owner) {
        ext[lane] = r < 0 ? INT32_MAX : (int32_t)r;              // a -1 sorts behind every row
        for (int q = 0; q < ROWS; ++q) a[lane * PITCH + q] = 0.0;
    }
    __syncthreads();
    if (r >= 0) {
        const long long sr = r >> 6, at = m.soff[sr] + (r & 63);
        const int wid = m.width[sr];
        int n = m.len[r];
        n = n < wid ? n : wid;
        for (int e = 0; e < n; ++e) {
            const long long c = m.col[at + 64LL * e];
            int q = -1;
            if (c >= first && c < first + cnt) {
                q = (int)(c - first);
            } else {
                int lo = cnt, hi = ROWS;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (ext[mid] < c) lo = mid + 1; else hi = mid;
                }
                if (lo < ROWS && ext[lo] == c) q = lo;
            }
            if (q >= 0) a[lane * PITCH + q] += m.val[at + 64LL * e];
        }
    }
    if (owner) {
        const double d = r >= 0 ? (m.dvec ? m.dvec[r] : m.dconst) : 1.0;
        for (int q = 0; q < ROWS; ++q) {
            const double dq = q == lane ? d : 0.0;
            a[lane * PITCH + q] = r >= 0 ? dq + m.c * a[lane * PITCH + q] : dq;
        }
    }
    __syncthreads();
    bool used = false, unusable = false;
    for (int k = 0; k < ROWS; ++k) {                             // uniform
        const double f = owner ? a[lane * PITCH + k] : 0.0;
        const double mag = __builtin_fabs(f);
        double key = !owner ? -2.0 : used ? -1.0 : (mag != mag ? __builtin_inf() : mag);
        int who = lane;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double okey = __shfl_xor(key, off, 64);
            const int owho = __shfl_xor(who, off, 64);
            if (okey > key || (okey == key && owho < who)) { key = okey; who = owho; }
        }
        const double pv = __shfl(f, who, 64);
        if (!(pv != 0.0 && __builtin_isfinite(pv))) unusable = true;
        const double pinv = 1.0 / pv;
        const bool mine = lane == who;
        if (mine) { used = true; who_of[k] = lane; step_of[lane] = k; }
        if (owner) prow[lane] = lane == k ? pinv : a[who * PITCH + lane] * pinv;
        __syncthreads();
        if (owner) {
            for (int j = 0; j < ROWS; ++j) {
                const double old = j == k ? 0.0 : a[lane * PITCH + j];
                a[lane * PITCH + j] = mine ? prow[j] : __builtin_fma(-f, prow[j], old);
            }
        }
        __syncthreads();
    }
    if (owner)
        for (int j = 0; j < ROWS; ++j)
            if (!__builtin_isfinite(a[lane * PITCH + j])) unusable = true;
    const bool bad = __any(unusable);
    if (lane == 0) { p.counts[B] = bad ? 1.0 : 0.0; if (counts_t) counts_t[B] = bad ? 1.0 : 0.0; }
    const bool kept = i_out < cnt;
    const int wi = kept ? who_of[i_out] : 0, si = kept ? step_of[i_out] : 0;
    for (int q = q_out; q < ROWS; q += bps) {
        w[64LL * q] = kept ? a[wi * PITCH + step_of[q]] : 0.0;
        if (wt) wt[64LL * q] = kept ? a[who_of[q] * PITCH + si] : 0.0;
    }
}

// out = P in, or (acc) acc += P in.  A wave serves the 64 rows of a slice, 64 / NB blocks: it gathers in[ext[q]] of each block once into
// LDS (0.0 at a -1), then z_lane = sum_q W[.., q, lane] * gathered[block of the lane][q], q ascending with fma.
template <int ROWS>
__global__ void __launch_bounds__(256) krylov_schwarz_apply_kernel(long long nrows, const KrylovSchwarz p, const int32_t* table,
                                                                   const double* in, double* out, double* acc, const KrylovScalars* sc,
                                                                   int always) {
    if (!always && sc->done) return;                             // uniform: the whole grid
    constexpr int PITCH = ROWS + 1;                              // the blocks of a wave read different banks
    __shared__ double gathered[4][8 * PITCH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nb = p.nb, bps = 64 / nb;
    const long long s = (long long)blockIdx.x * 4 + wave;
    const bool active = s * 64 < nrows;                          // wave-uniform
    if (active) {
        for (int t = lane; t < bps * ROWS; t += 64) {
            const int b = t / ROWS, q = t - b * ROWS;
            const long long B = s * bps + b, first = B * nb, left = nrows - first;
            const int cnt = left <= 0 ? 0 : left < nb ? (int)left : nb;
            const long long r = cnt ? krylov_schwarz_ext(table, B, ROWS, q, first, cnt, nrows) : -1;
            gathered[wave][b * PITCH + q] = r >= 0 ? in[r] : 0.0;
        }
    }
    __syncthreads();
    if (!active) return;
    const long long row = s * 64 + lane;
    const double* w = p.W + (s * ROWS) * 64 + lane;
    const double* g = gathered[wave] + (lane / nb) * PITCH;
    double z = 0.0;
#pragma unroll 8
    for (int q = 0; q < ROWS; ++q) z = __builtin_fma(w[64LL * q], g[q], z);
    if (row < nrows) {
        if (acc) acc[row] = acc[row] + z;
        else out[row] = z;
    }
}

static void krylov_schwarz_apply(const KrylovSchwarz& p, const int32_t* table, long long nrows, const double* in, double* out, double* acc,
                                 const KrylovScalars* sc, int always, hipStream_t s) {
    const dim3 grid((unsigned)((nrows + 255) / 256));
    if (p.rows == 32) hipLaunchKernelGGL(krylov_schwarz_apply_kernel<32>, grid, dim3(256), 0, s, nrows, p, table, in, out, acc, sc, always);
    else hipLaunchKernelGGL(krylov_schwarz_apply_kernel<64>, grid, dim3(256), 0, s, nrows, p, table, in, out, acc, sc, always);
}

static int krylov_schwarz_arguments(const char* who, int64_t nrows, int64_t nslices, int block, int rows, const void* table,
                                    const void* planes) {
    if (block != 8 && block != 16 && block != 32) { set_error(std::string(who) + ": block must be 8, 16 or 32"); return WLSQM_EVALUE; }
    if ((rows != 32 && rows != 64) || rows <= block) {
        set_error(std::string(who) + ": rows must be 32 or 64, and more than block");
        return WLSQM_EVALUE;
    }
    if (!table || !planes) { set_error(std::string(who) + ": null array"); return WLSQM_EVALUE; }
    if (nrows < 1 || nslices != (nrows + 63) / 64) { set_error(std::string(who) + ": nslices must be ceil(nrows / 64)"); return WLSQM_EVALUE; }
    if (nslices * (64 / block) > 0x7fffffffLL) { set_error(std::string(who) + ": too many blocks for one launch"); return WLSQM_EVALUE; }
    return WLSQM_OK;
}

// ---- coupled fields: m unknowns per point, block (a, b) of M = D_ab + sum_o coupling[a][b][o] A_o ------------------
// The unknowns are interleaved, x[point * m + a], so that a neighbour's m values are one contiguous load of 8 m bytes (16-byte loads
// for m = 2 and 4, which the entry points check the alignment for).  One wave per slice, one lane per point, m accumulators per lane.
// The order of operations, which tests/_krylov_system_ref.py states in numpy: per stored entry, in entry order,
//   t_ab  = coupling[a][b][0] * val_0, then t_ab = fma(coupling[a][b][o], val_o, t_ab) for o = 1 .. nop - 1
//   acc_a = fma(t_ab, x_b, acc_a) for b = 0 .. m - 1
// and at the end of the row  y_a = acc_a + s_a,  s_a = D_a0 x_0, then s_a = fma(D_ab, x_b, s_a) for b = 1 .. m - 1, x the point's own.
// The lane's terms of a dot product are added for a = 0 .. m - 1 in turn and then go through block_sums' tree.  The vectors of the
// recurrence are KrylovWork's at nrows = m npoints, and the update and reduce kernels above serve them unchanged: the product's
// launches write ceil(npoints / 256) partials per plane, the updates' ceil(m npoints / 256), and each reduce is handed the count of
// the launch that wrote.
// M^T is the same kind of system: block (a, b) of M^T is D_ba + sum_o coupling[b][a][o] A_o^T, so the same kernels
// serve it on the transposed arrays of the planes, with coupling and dconst exchanged on the host when KrylovCoupled is filled and a
// diag tensor read in place at the exchanged index (dswap).  The scalar diagonal holds the same numbers.

constexpr int KRYLOV_SYSTEM_FIELDS = 4;     // m <= 4
constexpr int KRYLOV_SYSTEM_PLANES = 8;     // nop <= 8: the coupling table is at most 4 * 4 * 8 = 128 doubles

struct KrylovCoupled {
    long long npoints, total;
    const int32_t* len; const int32_t* width; const long long* soff;
    const int32_t* col; const double* val;                      // plane o at val + o * total
    const double* dten;                                          // D_ab,i = dten ? dten[(a * m + b) * npoints + i] : dconst[a * m + b]
    int dswap;                                                   // M^T: dten is read at [(b * m + a) * npoints + i] (the host tables come exchanged)
    double dconst[KRYLOV_SYSTEM_FIELDS * KRYLOV_SYSTEM_FIELDS];
    double coupling[KRYLOV_SYSTEM_FIELDS * KRYLOV_SYSTEM_FIELDS * KRYLOV_SYSTEM_PLANES];   // [(a * m + b) * nop + o]
    const double* cpt;                                           // a per-point table (section 26): [((a * m + b) * nop + o) * npoints + i], else null
};

// The m unknowns of one point of an interleaved vector.
template <int M>
__device__ __forceinline__ void krylov_load_point(const double* at, double (&f)[M]) {
    if constexpr (M % 2 == 0) {
        krylov_load_fields<M>(at, f);
    } else {
#pragma unroll
        for (int b = 0; b < M; ++b) f[b] = at[b];
    }
}

// One stored entry: its nop values vs and the neighbour's unknowns xs into the lane's m sums.
template <int M, int NOP>
__device__ __forceinline__ void krylov_system_entry(const KrylovCoupled& q, const double (&vs)[NOP], const double (&xs)[M], double (&acc)[M]) {
#pragma unroll
    for (int a = 0; a < M; ++a) {
#pragma unroll
        for (int b = 0; b < M; ++b) {
            double t = q.coupling[(a * M + b) * NOP] * vs[0];
#pragma unroll
            for (int o = 1; o < NOP; ++o) t = __builtin_fma(q.coupling[(a * M + b) * NOP + o], vs[o], t);
            acc[a] = __builtin_fma(t, xs[b], acc[a]);
        }
    }
}

template <int M, int NOP>
__device__ __forceinline__ void krylov_system_row_sums(const KrylovCoupled& q, long long at, const double* x, int wid, int n, double (&acc)[M]) {
    constexpr int UNROLL = 4;
    const int32_t* col = q.col + at;
    const double* val = q.val + at;
#pragma unroll
    for (int a = 0; a < M; ++a) acc[a] = 0.0;
    for (int e = 0; e < wid; e += UNROLL) {                      // wave-uniform
        if (e + UNROLL <= n) {
            double xs[UNROLL][M], vs[UNROLL][NOP];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const long long c = col[64LL * (e + u)];
                krylov_load_point<M>(x + c * M, xs[u]);
#pragma unroll
                for (int o = 0; o < NOP; ++o) vs[u][o] = val[o * q.total + 64LL * (e + u)];
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) krylov_system_entry<M, NOP>(q, vs[u], xs[u], acc);
        } else {
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                if (e + u < n) {
                    const long long c = col[64LL * (e + u)];
                    double xs[M], vs[NOP];
                    krylov_load_point<M>(x + c * M, xs);
#pragma unroll
                    for (int o = 0; o < NOP; ++o) vs[o] = val[o * q.total + 64LL * (e + u)];
                    krylov_system_entry<M, NOP>(q, vs, xs, acc);
                }
            }
        }
    }
}

enum { SYSTEM_RESIDUAL = 0, SYSTEM_V = 1, SYSTEM_T = 2, SYSTEM_PRODUCT = 3 };

// y = M in.  `mode` is uniform over the grid:
//   RESIDUAL: out = out2 = b - y (w is b), partials (out, out) and (b, b)
//   V:        out = y, partial (w, out)                  (the second plane is written and not read)
//   T:        out = y, partials (out, w) and (out, out)
//   PRODUCT:  T whatever the state of a solve
template <int M, int NOP>
__global__ void __launch_bounds__(256) krylov_system_spmv_kernel(const KrylovCoupled q, int mode, const double* in, const double* w, double* out,
                                                                 double* out2, double* partial, const KrylovScalars* sc) {
    if (mode != SYSTEM_PRODUCT && sc->done) return;              // uniform: the whole grid
    const int lane = threadIdx.x & 63;
    const long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long row = s * 64 + lane;
    double pa = 0.0, pb = 0.0;
    if (s * 64 < q.npoints) {                                    // wave-uniform
        const int wid = __builtin_amdgcn_readfirstlane(q.width[s]);
        const long long at = q.soff[s] + lane;
        int n = row < q.npoints ? q.len[row] : 0;
        n = n < wid ? n : wid;
        double acc[M];
        krylov_system_row_sums<M, NOP>(q, at, in, wid, n, acc);
        if (row < q.npoints) {
            double xi[M], y[M], wi[M];
            krylov_load_point<M>(in + row * M, xi);
            krylov_load_point<M>(w + row * M, wi);
#pragma unroll
            for (int a = 0; a < M; ++a) {
                double sa = 0.0;
#pragma unroll
                for (int b = 0; b < M; ++b) {
                    const double d = q.dten ? q.dten[(q.dswap ? b * M + a : a * M + b) * q.npoints + row] : q.dconst[a * M + b];
                    sa = b == 0 ? d * xi[0] : __builtin_fma(d, xi[b], sa);
                }
                y[a] = acc[a] + sa;
            }
            if (mode == SYSTEM_RESIDUAL) {
#pragma unroll
                for (int a = 0; a < M; ++a) {
                    const double r = wi[a] - y[a];
                    out[row * M + a] = r; out2[row * M + a] = r;
                    pa += r * r; pb += wi[a] * wi[a];
                }
            } else {
#pragma unroll
                for (int a = 0; a < M; ++a) {
                    out[row * M + a] = y[a];
                    pa += wi[a] * y[a]; pb += y[a] * y[a];
                }
            }
        }
    }
    block_sums<true>(pa, pb, partial, gridDim.x);
}

// dinv[i * m + a] = 1 / (D_aa,i + sum_o coupling[a][a][o] own_o), own_o the sum of row i's entries in column i of plane o in entry order
// (plain sums, two roundings per term, o ascending from coupling[a][a][0] * own_0); the partial counts the points with an unusable entry.
template <int M, int NOP>
__global__ void __launch_bounds__(256) krylov_system_diag_kernel(const KrylovCoupled q, double* dinv, double* partial) {
    const int lane = threadIdx.x & 63;
    const long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long row = s * 64 + lane;
    double bad = 0.0;
    if (s * 64 < q.npoints) {                                    // wave-uniform
        const int wid = __builtin_amdgcn_readfirstlane(q.width[s]);
        const long long at = q.soff[s] + lane;
        int n = row < q.npoints ? q.len[row] : 0;
        n = n < wid ? n : wid;
        double own[NOP];
#pragma unroll
        for (int o = 0; o < NOP; ++o) own[o] = 0.0;
        for (int e = 0; e < wid; ++e) {                          // wave-uniform
            if (e < n && q.col[at + 64LL * e] == row) {
#pragma unroll
                for (int o = 0; o < NOP; ++o) own[o] += q.val[o * q.total + at + 64LL * e];
            }
        }
        if (row < q.npoints) {
            bool unusable = false;
#pragma unroll
            for (int a = 0; a < M; ++a) {
                double t = q.coupling[(a * M + a) * NOP] * own[0];
#pragma unroll
                for (int o = 1; o < NOP; ++o) t = t + q.coupling[(a * M + a) * NOP + o] * own[o];
                const double diag = (q.dten ? q.dten[(a * M + a) * q.npoints + row] : q.dconst[a * M + a]) + t;
                const bool ok = diag != 0.0 && __builtin_isfinite(diag);
                dinv[row * M + a] = ok ? 1.0 / diag : 0.0;
                unusable = unusable || !ok;
            }
            bad = unusable ? 1.0 : 0.0;
        }
    }
    block_sums<false>(bad, 0.0, partial, gridDim.x);
}

// The gradients of a loss through the coupled solve M x = b, lam the solution of M^T lam = dL/dx, in one pass
// over the forward structure with krylov_system_spmv_kernel's mapping.  The order of operations, which
// tests/_krylov_system_adjoint_ref.py states in numpy:
//   per lane, once:  u[b][o] = c[0][b][o] * lam_0, then u[b][o] = fma(c[a][b][o], lam_a, u[b][o]) for a = 1 .. m - 1   (lam the row's own)
//   VALUES (nop, total): per live entry in entry order, per plane o: t = u[0][o] * x_0, then t = fma(u[b][o], x_b, t) for b = 1 .. m - 1,
//           x the unknowns of the entry's column; gval[o * total + at + 64 e] = -t.  +0.0 in every padding position of every plane, the
//           lanes of rows beyond npoints included; their padding col is never loaded, and val is never loaded at all
//   DIAG (m, m, npoints): gdiag[(a * m + b) * npoints + j] = -(lam[j][a] * x[j][b]), one rounding
// Each output is a template flag: a pass without VALUES never stores into a plane.  No atomics, no scratch, no workspace.
// POINT: c[a][b][o] is the row's own, q.cpt[((a * m + b) * nop + o) * npoints + j], one coalesced run per (a, b, o).
template <int M, int NOP>
__device__ __forceinline__ void krylov_system_grads_entry(const double (&u)[M][NOP], const double (&xs)[M], double* out, long long total) {
#pragma unroll
    for (int o = 0; o < NOP; ++o) {
        double t = u[0][o] * xs[0];
#pragma unroll
        for (int b = 1; b < M; ++b) t = __builtin_fma(u[b][o], xs[b], t);
        out[o * total] = -t;
    }
}

template <int M, int NOP, bool VALUES, bool DIAG, bool POINT = false>
__global__ void __launch_bounds__(256) krylov_system_grads_kernel(const KrylovCoupled q, const double* lam, const double* x, double* gval,
                                                                  double* gdiag) {
    const int lane = threadIdx.x & 63;
    const long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long row = s * 64 + lane;
    if (s * 64 >= q.npoints) return;                             // wave-uniform
    const bool live = row < q.npoints;
    double lj[M];
#pragma unroll
    for (int a = 0; a < M; ++a) lj[a] = 0.0;
    if (live) krylov_load_point<M>(lam + row * M, lj);
    if (DIAG && live) {
        double xj[M];
        krylov_load_point<M>(x + row * M, xj);
#pragma unroll
        for (int a = 0; a < M; ++a) {
#pragma unroll
            for (int b = 0; b < M; ++b) gdiag[(a * M + b) * q.npoints + row] = -(lj[a] * xj[b]);
        }
    }
    if (VALUES) {
        constexpr int UNROLL = 4;
        const int wid = __builtin_amdgcn_readfirstlane(q.width[s]);
        const long long at = q.soff[s] + lane;
        int n = live ? q.len[row] : 0;
        n = n < wid ? n : wid;
        const int32_t* col = q.col + at;
        double* out = gval + at;
        double u[M][NOP];
#pragma unroll
        for (int b = 0; b < M; ++b) {
#pragma unroll
            for (int o = 0; o < NOP; ++o) {
                double t;
                if constexpr (POINT) {                           // a lane beyond npoints has lam = 0 and stores only padding zeros
                    const double* cp = q.cpt + (live ? row : 0);
                    t = cp[(b * NOP + o) * q.npoints] * lj[0];
#pragma unroll
                    for (int a = 1; a < M; ++a) t = __builtin_fma(cp[((a * M + b) * NOP + o) * q.npoints], lj[a], t);
                } else {
                    t = q.coupling[b * NOP + o] * lj[0];
#pragma unroll
                    for (int a = 1; a < M; ++a) t = __builtin_fma(q.coupling[(a * M + b) * NOP + o], lj[a], t);
                }
                u[b][o] = t;
            }
        }
        for (int e = 0; e < wid; e += UNROLL) {                  // wave-uniform
            if (e + UNROLL <= n) {
                double xs[UNROLL][M];
#pragma unroll
                for (int k = 0; k < UNROLL; ++k) {
                    const long long c = col[64LL * (e + k)];
                    krylov_load_point<M>(x + c * M, xs[k]);
                }
#pragma unroll
                for (int k = 0; k < UNROLL; ++k) krylov_system_grads_entry<M, NOP>(u, xs[k], out + 64LL * (e + k), q.total);
            } else {
                for (int k = 0; k < UNROLL && e + k < wid; ++k) {
                    if (e + k < n) {
                        const long long c = col[64LL * (e + k)];
                        double xs[M];
                        krylov_load_point<M>(x + c * M, xs);
                        krylov_system_grads_entry<M, NOP>(u, xs, out + 64LL * (e + k), q.total);
                    } else {
#pragma unroll
                        for (int o = 0; o < NOP; ++o) out[o * q.total + 64LL * (e + k)] = 0.0;
                    }
                }
            }
        }
    }
}

template <int M, int NOP>
static void krylov_system_grads_run(const KrylovCoupled& q, const double* lam, const double* x, double* gval, double* gdiag, hipStream_t s) {
    const dim3 grid((unsigned)((q.npoints + 255) / 256)), block(256);
    if (q.cpt) {
        if (gdiag) hipLaunchKernelGGL((krylov_system_grads_kernel<M, NOP, true, true, true>), grid, block, 0, s, q, lam, x, gval, gdiag);
        else hipLaunchKernelGGL((krylov_system_grads_kernel<M, NOP, true, false, true>), grid, block, 0, s, q, lam, x, gval, gdiag);
    } else if (gdiag) hipLaunchKernelGGL((krylov_system_grads_kernel<M, NOP, true, true>), grid, block, 0, s, q, lam, x, gval, gdiag);
    else hipLaunchKernelGGL((krylov_system_grads_kernel<M, NOP, true, false>), grid, block, 0, s, q, lam, x, gval, gdiag);
}

template <int M>
static void krylov_system_grads_planes(int nop, const KrylovCoupled& q, const double* lam, const double* x, double* gval, double* gdiag,
                                       hipStream_t s) {
    if (!gval) {                                                 // DIAG alone does not look at the planes: one instance per m
        hipLaunchKernelGGL((krylov_system_grads_kernel<M, 1, false, true>), dim3((unsigned)((q.npoints + 255) / 256)), dim3(256), 0, s, q,
                           lam, x, gval, gdiag);
        return;
    }
    switch (nop) {
    case 1: krylov_system_grads_run<M, 1>(q, lam, x, gval, gdiag, s); break;
    case 2: krylov_system_grads_run<M, 2>(q, lam, x, gval, gdiag, s); break;
    case 3: krylov_system_grads_run<M, 3>(q, lam, x, gval, gdiag, s); break;
    case 4: krylov_system_grads_run<M, 4>(q, lam, x, gval, gdiag, s); break;
    case 5: krylov_system_grads_run<M, 5>(q, lam, x, gval, gdiag, s); break;
    case 6: krylov_system_grads_run<M, 6>(q, lam, x, gval, gdiag, s); break;
    case 7: krylov_system_grads_run<M, 7>(q, lam, x, gval, gdiag, s); break;
    default: krylov_system_grads_run<M, 8>(q, lam, x, gval, gdiag, s); break;
    }
}

// ---- blocks over points for coupled fields: P = blockdiag(M_BB)^-1, block B the points B points .. (B + 1) points - 1 --
// with all m unknowns of each: R = m points <= 32 consecutive rows of the flat vectors.  Section 19's plane carried to R <= NB, NB the
// smallest of 8, 16, 32 that holds R: a wave holds G = 64 / NB blocks, lane g NB + l is row l of block wave G + g, flat row
// (wave G + g) R + l, live when l < R and the row is below m npoints.  W[(wave NB + j) 64 + lane] is entry (l, j) of that block's inverse;
// rows and columns from R on, and the rows that the cut last block leaves over, hold the identity.  Behind the nwaves NB 64 doubles sit
// ceil(nwaves / 4) per-workgroup counts of the unusable blocks, which every start reduces into status 4.  A block of points need not
// stay inside one slice of the operator, so every lane looks up the slice of its own point.
// The entries, which tests/_krylov_system_block_ref.py states in numpy: entry ((i, a), (j, b)) = D_ab,i delta_ij + s, s the plain sum over
// the stored entries e of row i with column j, in entry order, of t_ab(e) = c[a][b][0] val_0, then fma(c[a][b][o], val_o, t) for
// o = 1 .. nop - 1; c the constant table or the point's own coefficients c[a][b][o][i].  The blocks of M^T are the transposes: the
// factor always reads the forward arrays and writes the transposed inverses into WT.

__host__ __device__ static inline int krylov_system_block_nb(int rows) { return rows <= 8 ? 8 : rows <= 16 ? 16 : 32; }

static long long krylov_system_block_waves(long long npoints, int m, int points) {
    const long long nblocks = (npoints + points - 1) / points;
    const int per = 64 / krylov_system_block_nb(m * points);
    return (nblocks + per - 1) / per;
}

// t_ab(e) of the lane's own a.  The constant table is indexed wave-uniformly (every a in turn, the lane keeps its own); a per-point
// table is read at the lane's own address.
__device__ __forceinline__ double krylov_system_block_term(const KrylovCoupled& q, int m, int nop, int a, int b, long long i,
                                                           const double (&vs)[KRYLOV_SYSTEM_PLANES]) {
    if (q.cpt) {
        const double* cp = q.cpt + ((long long)(a * m + b) * nop) * q.npoints + i;
        double t = cp[0] * vs[0];
#pragma unroll
        for (int o = 1; o < KRYLOV_SYSTEM_PLANES; ++o)
            if (o < nop) t = __builtin_fma(cp[o * q.npoints], vs[o], t);
        return t;
    }
    double t = 0.0;
    for (int aa = 0; aa < m; ++aa) {                             // uniform
        const int at = (aa * m + b) * nop;
        double ta = q.coupling[at] * vs[0];
#pragma unroll
        for (int o = 1; o < KRYLOV_SYSTEM_PLANES; ++o)
            if (o < nop) ta = __builtin_fma(q.coupling[at + o], vs[o], ta);
        t = aa == a ? ta : t;
    }
    return t;
}

// One lane per row of the block layout.  The lane gathers its row of the block (the m targets of every stored entry whose column is a
// point of the block, in entry order; padding is beyond the lane's own count and never loaded), then the NB lanes of a block invert it
// exactly as krylov_blocks_kernel does, with the same elimination, checks, counts and stores.  m, nop and points are run-time
// arguments; every register index is a constant.  invert == 0 stores the gathered rows as they are and counts nothing.
template <int NB>
__global__ void __launch_bounds__(256) krylov_system_blocks_kernel(const KrylovCoupled q, int m, int nop, int points, long long nwaves,
                                                                   int invert, double* W, double* WT) {
    constexpr int G = 64 / NB;
    const int lane = threadIdx.x & 63, l = lane & (NB - 1), b0 = lane - l;
    const long long wv = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    double bad = 0.0;
    if (wv < nwaves) {                                           // wave-uniform
        const int rows = m * points;
        const long long blk = wv * G + lane / NB, row = blk * rows + l;
        const bool live = l < rows && row < q.npoints * m;
        const long long i = live ? row / m : 0, first = blk * points;        // the lane's point; the block's first point
        const int a = live ? (int)(row - i * m) : 0;
        double A[NB], inv[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) A[j] = 0.0;
        if (live) {
            const long long sl = i >> 6, at = q.soff[sl] + (i & 63);
            const int wid = q.width[sl];
            int n = q.len[i];
            n = n < wid ? n : wid;
            for (int e = 0; e < n; ++e) {
                const long long p = (long long)q.col[at + 64LL * e] - first;
                if (p >= 0 && p < points) {
                    double vs[KRYLOV_SYSTEM_PLANES];
#pragma unroll
                    for (int o = 0; o < KRYLOV_SYSTEM_PLANES; ++o) vs[o] = o < nop ? q.val[o * q.total + at + 64LL * e] : 0.0;
                    for (int b = 0; b < m; ++b) {                // uniform
                        const double t = krylov_system_block_term(q, m, nop, a, b, i, vs);
                        const int tj = (int)p * m + b;
#pragma unroll
                        for (int j = 0; j < NB; ++j) A[j] += tj == j ? t : 0.0;
                    }
                }
            }
            for (int b = 0; b < m; ++b) {                        // uniform
                double d = 0.0;
                if (q.dten) {
                    d = q.dten[(long long)(a * m + b) * q.npoints + i];
                } else {
                    for (int aa = 0; aa < m; ++aa) d = aa == a ? q.dconst[aa * m + b] : d;
                }
                const int tj = (int)(i - first) * m + b;
#pragma unroll
                for (int j = 0; j < NB; ++j) A[j] = (tj == j ? d : 0.0) + A[j];
            }
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            if (!live) A[j] = j == l ? 1.0 : 0.0;
            inv[j] = j == l ? 1.0 : 0.0;
        }
        double* w = W + (wv * NB) * 64 + lane;
        if (!invert) {                                           // uniform: the gathered blocks as they are (wlsqm_hip_krylov_system_block_gather_device)
#pragma unroll
            for (int j = 0; j < NB; ++j) w[64LL * j] = A[j];
        } else {
            bool used = false, unusable = false;
            int step = 0;
            krylov_eliminate<NB, 0>(A, inv, lane, used, step, unusable);
            int src = lane;
#pragma unroll
            for (int j = 0; j < NB; ++j)
                if (__shfl(step, b0 + j, 64) == l) src = b0 + j;
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                inv[j] = __shfl(inv[j], src, 64);
                if (!__builtin_isfinite(inv[j])) unusable = true;
                w[64LL * j] = inv[j];
            }
            if (WT) {
                double* wt = WT + (wv * NB + l) * 64 + b0;       // column l of the transposed block, its rows b0 .. b0 + NB - 1
#pragma unroll
                for (int j = 0; j < NB; ++j) wt[j] = inv[j];
            }
            bad = unusable ? 1.0 : 0.0;
        }
    }
    double* counts = W + nwaves * NB * 64;
    block_sums<false>(bad, 0.0, counts, gridDim.x);
    if (WT && threadIdx.x == 0) WT[nwaves * NB * 64 + blockIdx.x] = counts[blockIdx.x];
}

// krylov_update_block_kernel's P and S steps under the (wave, g, l) mapping above: no partial sums, so no summation order changes.
template <int NB, int MODE>
__global__ void __launch_bounds__(256) krylov_system_update_block_kernel(long long nrows, int rows, long long nwaves, const KrylovWork k,
                                                                         const double* W, const KrylovScalars* sc) {
    if (sc->done) return;                                        // uniform: the whole grid
    const int lane = threadIdx.x & 63, l = lane & (NB - 1);
    const long long wv = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wv >= nwaves) return;                                    // wave-uniform
    const long long i = (wv * (64 / NB) + lane / NB) * rows + l;
    const bool live = l < rows && i < nrows;
    double u = 0.0;
    if (live) {
        if (MODE == UPDATE_P) {
            u = k.r[i];
            if (sc->iterations > 0) {
                const double omega = sc->omega, beta = (sc->rho / sc->rho_old) * (sc->alpha / omega);
                u = u + beta * (k.p[i] - omega * k.v[i]);
            }
            k.p[i] = u;
        } else {
            u = k.r[i] - sc->alpha * k.v[i];
            k.s[i] = u;
        }
    }
    const double z = krylov_block_apply<NB>(W + (wv * NB) * 64 + lane, u, lane);
    if (live) (MODE == UPDATE_P ? k.phat : k.shat)[i] = z;
}

template <int NB>
__global__ void __launch_bounds__(256) krylov_system_precondition_kernel(long long nrows, int rows, long long nwaves, const double* W,
                                                                         const double* v, double* out) {
    const int lane = threadIdx.x & 63, l = lane & (NB - 1);
    const long long wv = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wv >= nwaves) return;                                    // wave-uniform
    const long long i = (wv * (64 / NB) + lane / NB) * rows + l;
    const bool live = l < rows && i < nrows;
    const double z = krylov_block_apply<NB>(W + (wv * NB) * 64 + lane, live ? v[i] : 0.0, lane);
    if (live) out[i] = z;
}

// The P or S step of an iteration with the blocks over `points` points.
template <int MODE>
static void krylov_system_update_block(long long npoints, int m, int points, const KrylovWork& w, const double* W, hipStream_t s) {
    const int rows = m * points;
    const long long nrows = npoints * m, nwaves = krylov_system_block_waves(npoints, m, points);
    const dim3 grid((unsigned)((nwaves + 3) / 4)), block(256);
    const KrylovScalars* sc = w.sc;
    switch (krylov_system_block_nb(rows)) {
    case 8: hipLaunchKernelGGL((krylov_system_update_block_kernel<8, MODE>), grid, block, 0, s, nrows, rows, nwaves, w, W, sc); break;
    case 16: hipLaunchKernelGGL((krylov_system_update_block_kernel<16, MODE>), grid, block, 0, s, nrows, rows, nwaves, w, W, sc); break;
    default: hipLaunchKernelGGL((krylov_system_update_block_kernel<32, MODE>), grid, block, 0, s, nrows, rows, nwaves, w, W, sc); break;
    }
}

// The start of a solve with the blocks: the counts behind the plane into status 4, in the scalar diagonal's place.
static void krylov_system_block_counts(long long npoints, int m, int points, const KrylovWork& w, const double* W, double rtol, double atol,
                                       int maxiter, hipStream_t s) {
    const long long nwaves = krylov_system_block_waves(npoints, m, points);
    const double* counts = W + nwaves * krylov_system_block_nb(m * points) * 64;
    hipLaunchKernelGGL(krylov_reduce_kernel, dim3(1), dim3(256), 0, s, (int)REDUCE_DIAG, counts, (nwaves + 3) / 4, 1, w.sc, rtol, atol, maxiter);
}

// The checks of `points` and of a plane that the block entry points share, ahead of any launch.
static int krylov_system_block_arguments(const char* who, int m, int points, const void* planes, const void* planes_t) {
    const std::string name(who);
    if (m < 1 || m > KRYLOV_SYSTEM_FIELDS) { set_error(name + ": m must be 1 .. 4"); return WLSQM_EVALUE; }
    if (points < 1 || m * points > 32) {
        set_error(name + ": points must be 1 .. " + std::to_string(32 / m) + " for m = " + std::to_string(m) + " (m points <= 32)");
        return WLSQM_EVALUE;
    }
    if (!planes) { set_error(name + ": null array"); return WLSQM_EVALUE; }
    if (m % 2 == 0 && (((uintptr_t)planes | (uintptr_t)planes_t) & 15)) {
        set_error(name + ": with m = 2 or 4 the block planes must be 16-byte aligned");
        return WLSQM_EVALUE;
    }
    return WLSQM_OK;
}

enum { SYSTEM_CALL_START = 0, SYSTEM_CALL_ITERATE = 1, SYSTEM_CALL_PRODUCT = 2 };

struct KrylovSystemCall {
    int points = 0; const double* W = nullptr;                  // blocks over points (section 27): the plane, else null
    int what, jacobi, maxiter;
    KrylovCoupled q;
    KrylovWork w;                                               // at nrows = m npoints
    const double *in, *other;                                   // start: x and b; product: in and w
    double* x;                                                  // iterate: x; product: out
    double rtol, atol;
    int64_t niter;
    hipStream_t s;
};

template <int M, int NOP>
static void krylov_system_run(const KrylovSystemCall& c) {
    const KrylovWork& w = c.w;
    const long long nwgp = (c.q.npoints + 255) / 256, nrows = c.q.npoints * M;
    const dim3 pgrid((unsigned)nwgp), ugrid((unsigned)w.nwg), block(256);
    const KrylovScalars* sc = w.sc;
    hipStream_t s = c.s;
    double* const none = nullptr;
    if (c.what == SYSTEM_CALL_START) {
        if (c.W) {
            krylov_system_block_counts(c.q.npoints, M, c.points, w, c.W, c.rtol, c.atol, c.maxiter, s);
        } else {
            if (c.jacobi) {
                hipLaunchKernelGGL((krylov_system_diag_kernel<M, NOP>), pgrid, block, 0, s, c.q, w.dinv, w.partial);
                note_kernel("krylov-system-diag");
            }
            krylov_reduce(REDUCE_DIAG, w, c.jacobi ? nwgp : 0, 1, c.rtol, c.atol, c.maxiter, s);
        }
        hipLaunchKernelGGL((krylov_system_spmv_kernel<M, NOP>), pgrid, block, 0, s, c.q, (int)SYSTEM_RESIDUAL, c.in, c.other, w.r, w.r0, w.partial, sc);
        note_kernel("krylov-system-spmv");
        krylov_reduce(REDUCE_RESIDUAL, w, nwgp, 2, c.rtol, c.atol, c.maxiter, s);
        note_kernel("krylov-reduce");
    } else if (c.what == SYSTEM_CALL_ITERATE) {
        for (int64_t it = 0; it < c.niter; ++it) {
            if (c.W) krylov_system_update_block<UPDATE_P>(c.q.npoints, M, c.points, w, c.W, s);
            else hipLaunchKernelGGL((krylov_update_kernel<UPDATE_P>), ugrid, block, 0, s, nrows, w, c.x, sc);
            hipLaunchKernelGGL((krylov_system_spmv_kernel<M, NOP>), pgrid, block, 0, s, c.q, (int)SYSTEM_V, (const double*)w.phat, (const double*)w.r0, w.v, none, w.partial, sc);
            krylov_reduce(REDUCE_ALPHA, w, nwgp, 1, 0.0, 0.0, 0, s);
            if (c.W) krylov_system_update_block<UPDATE_S>(c.q.npoints, M, c.points, w, c.W, s);
            else hipLaunchKernelGGL((krylov_update_kernel<UPDATE_S>), ugrid, block, 0, s, nrows, w, c.x, sc);
            hipLaunchKernelGGL((krylov_system_spmv_kernel<M, NOP>), pgrid, block, 0, s, c.q, (int)SYSTEM_T, (const double*)w.shat, (const double*)w.s, w.t, none, w.partial, sc);
            krylov_reduce(REDUCE_OMEGA, w, nwgp, 2, 0.0, 0.0, 0, s);
            hipLaunchKernelGGL((krylov_update_kernel<UPDATE_X>), ugrid, block, 0, s, nrows, w, c.x, sc);
            krylov_reduce(REDUCE_RHO, w, w.nwg, 2, 0.0, 0.0, 0, s);
        }
        note_kernel(c.W ? "krylov-system-update-block" : "krylov-update");
    } else {
        hipLaunchKernelGGL((krylov_system_spmv_kernel<M, NOP>), pgrid, block, 0, s, c.q, (int)SYSTEM_PRODUCT, c.in, c.other, c.x, none, w.partial, sc);
        krylov_reduce(REDUCE_PRODUCT, w, nwgp, 2, 0.0, 0.0, 0, s);
        note_kernel("krylov-system-spmv");
    }
}

template <int M>
static void krylov_system_planes(int nop, const KrylovSystemCall& c) {
    switch (nop) {
    case 1: krylov_system_run<M, 1>(c); break;
    case 2: krylov_system_run<M, 2>(c); break;
    case 3: krylov_system_run<M, 3>(c); break;
    case 4: krylov_system_run<M, 4>(c); break;
    case 5: krylov_system_run<M, 5>(c); break;
    case 6: krylov_system_run<M, 6>(c); break;
    case 7: krylov_system_run<M, 7>(c); break;
    default: krylov_system_run<M, 8>(c); break;
    }
}

// The checks and the kernel argument that the three entry points share, then the call's launches.
static int krylov_system_call(const char* who, KrylovSystemCall& c, int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                              const int64_t* soff, const int32_t* col, const double* val, int64_t total, int nop, int m,
                              const double* coupling, const double* diag, const double* diag_const, void* workspace, int device,
                              bool transposed = false) {
    const std::string name(who);
    if (m < 1 || m > KRYLOV_SYSTEM_FIELDS) { set_error(name + ": m must be 1 .. 4"); return WLSQM_EVALUE; }
    if (nop < 1 || nop > KRYLOV_SYSTEM_PLANES) { set_error(name + ": nop must be 1 .. 8"); return WLSQM_EVALUE; }
    if (npoints < 1 || nslices < 0 || npoints > 64 * nslices || total < 0 || (npoints * m + 255) / 256 > 0x7fffffffLL) {
        set_error(name + ": npoints must be 1 .. 64 * nslices");
        return WLSQM_EVALUE;
    }
    if (!len || !width || !soff || !col || !val || !coupling || !workspace || (!diag && !diag_const) || !c.in || !c.other || !c.x) {
        set_error(name + ": null array");
        return WLSQM_EVALUE;
    }
    if (m % 2 == 0 && (((uintptr_t)c.in | (uintptr_t)c.other | (uintptr_t)c.x | (uintptr_t)workspace) & 15)) {
        set_error(name + ": with m = 2 or 4 the vectors and the workspace must be 16-byte aligned");
        return WLSQM_EVALUE;
    }
    KrylovCoupled& q = c.q;
    q.npoints = npoints; q.total = total;
    q.len = len; q.width = width; q.soff = reinterpret_cast<const long long*>(soff);
    q.col = col; q.val = val; q.dten = diag; q.dswap = transposed ? 1 : 0; q.cpt = nullptr;
    for (int i = 0; i < KRYLOV_SYSTEM_FIELDS * KRYLOV_SYSTEM_FIELDS; ++i) q.dconst[i] = (!diag && i < m * m) ? diag_const[i] : 0.0;
    for (int i = 0; i < KRYLOV_SYSTEM_FIELDS * KRYLOV_SYSTEM_FIELDS * KRYLOV_SYSTEM_PLANES; ++i) q.coupling[i] = i < m * m * nop ? coupling[i] : 0.0;
    if (transposed) {                                           // block (a, b) of M^T takes D_ba and coupling[b][a][:]
        for (int a = 0; a < m; ++a) {
            for (int b = 0; b < m; ++b) {
                if (!diag) q.dconst[a * m + b] = diag_const[b * m + a];
                for (int o = 0; o < nop; ++o) q.coupling[(a * m + b) * nop + o] = coupling[(b * m + a) * nop + o];
            }
        }
    }
    DeviceScope scope;
    const int rc = scope.enter(device);
    if (rc != WLSQM_OK) return rc;
    c.w = krylov_work(workspace, npoints * m, c.jacobi != 0);
    switch (m) {
    case 1: krylov_system_planes<1>(nop, c); break;
    case 2: krylov_system_planes<2>(nop, c); break;
    case 3: krylov_system_planes<3>(nop, c); break;
    default: krylov_system_planes<4>(nop, c); break;
    }
    WLSQM_HIP_CHECK(hipGetLastError());
    return WLSQM_OK;
}

// ---- a per-point coupling: M[(i, a), (j, b)] = D_ab,i delta_ij + sum_o c[a][b][o][i] A_o[i, j] ----------------------
// c is a device tensor (m, m, nop, npoints), plane-major like the diag tensor: the equation of point i carries its own coefficients.
// m^2 nop coefficients per lane do not fit registers beside the product, so the order of operations is not section 24's; it is the one
// that tests/_krylov_system_point_ref.py states in numpy.
// Forward (krylov-system-spmv-point), section 24's mapping, nop m accumulators per lane:
//   per stored entry, in entry order:  s[o][b] = fma(val_o, x_b, s[o][b]), x the unknowns of the entry's column   (s = A_o x_b, row i)
//   at the end of the row:  t_a = c[a][0][0][i] * s[0][0], then t_a = fma(c[a][b][o][i], s[o][b], t_a), b outer and o inner, (0, 0) left out
//   y_a = t_a + s_a, s_a the diag part exactly as in section 24
// Each coefficient is one coalesced 512-byte run per (a, b, o), used once and dropped.
// Transposed: (M^T lam)_b(j) = (D^T lam)_b(j) + sum_o sum_i A_o^T[j, i] z[i][o][b], the coefficients applied at their own point:
//   krylov-system-mix, one lane per point:  z[i][o][b] = c[0][b][o][i] * lam_0, then fma(c[a][b][o][i], lam_a, .) for a = 1 .. m - 1,
//     written as (npoints, nop, m)
//   krylov-system-spmv-mixed on the operator's transposed arrays, m accumulators: per stored entry of row j, in entry order, o ascending,
//     acc_b = fma(valT_o, z[col][o][b], acc_b); y_b = acc_b + s_b, s_b = D_0b lam_0, then fma(D_ab, lam_a, s_b): dten at the exchanged index
// No coefficient is gathered.  The epilogues, block_sums and the partial counts are section 24's.

// The end of a row of either product: y = t + (the diag part), then the epilogue that `mode` names (krylov_system_spmv_kernel's).
template <int M>
__device__ __forceinline__ void krylov_system_finish(const KrylovCoupled& q, int mode, const double* in, const double* w, double* out, double* out2,
                                                     long long row, const double (&t)[M], double& pa, double& pb) {
    double xi[M], y[M], wi[M];
    krylov_load_point<M>(in + row * M, xi);
    krylov_load_point<M>(w + row * M, wi);
#pragma unroll
    for (int a = 0; a < M; ++a) {
        double sa = 0.0;
#pragma unroll
        for (int b = 0; b < M; ++b) {
            const double d = q.dten ? q.dten[(q.dswap ? b * M + a : a * M + b) * q.npoints + row] : q.dconst[a * M + b];
            sa = b == 0 ? d * xi[0] : __builtin_fma(d, xi[b], sa);
        }
        y[a] = t[a] + sa;
    }
    if (mode == SYSTEM_RESIDUAL) {
#pragma unroll
        for (int a = 0; a < M; ++a) {
            const double r = wi[a] - y[a];
            out[row * M + a] = r; out2[row * M + a] = r;
            pa += r * r; pb += wi[a] * wi[a];
        }
    } else {
#pragma unroll
        for (int a = 0; a < M; ++a) {
            out[row * M + a] = y[a];
            pa += wi[a] * y[a]; pb += y[a] * y[a];
        }
    }
}

template <int M, int NOP>
__device__ __forceinline__ void krylov_point_entry(const double (&vs)[NOP], const double (&xs)[M], double (&s)[NOP][M]) {
#pragma unroll
    for (int o = 0; o < NOP; ++o) {
#pragma unroll
        for (int b = 0; b < M; ++b) s[o][b] = __builtin_fma(vs[o], xs[b], s[o][b]);
    }
}

template <int M, int NOP>
__global__ void __launch_bounds__(256) krylov_system_spmv_point_kernel(const KrylovCoupled q, int mode, const double* in, const double* w, double* out,
                                                                       double* out2, double* partial, const KrylovScalars* sc) {
    if (mode != SYSTEM_PRODUCT && sc->done) return;              // uniform: the whole grid
    constexpr int UNROLL = M * NOP > 16 ? 2 : 4;
    const int lane = threadIdx.x & 63;
    const long long sl = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long row = sl * 64 + lane;
    double pa = 0.0, pb = 0.0;
    if (sl * 64 < q.npoints) {                                   // wave-uniform
        const int wid = __builtin_amdgcn_readfirstlane(q.width[sl]);
        const long long at = q.soff[sl] + lane;
        int n = row < q.npoints ? q.len[row] : 0;
        n = n < wid ? n : wid;
        const int32_t* col = q.col + at;
        const double* val = q.val + at;
        double s[NOP][M];
#pragma unroll
        for (int o = 0; o < NOP; ++o) {
#pragma unroll
            for (int b = 0; b < M; ++b) s[o][b] = 0.0;
        }
        for (int e = 0; e < wid; e += UNROLL) {                  // wave-uniform
            if (e + UNROLL <= n) {
                double xs[UNROLL][M], vs[UNROLL][NOP];
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    const long long c = col[64LL * (e + u)];
                    krylov_load_point<M>(in + c * M, xs[u]);
#pragma unroll
                    for (int o = 0; o < NOP; ++o) vs[u][o] = val[o * q.total + 64LL * (e + u)];
                }
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) krylov_point_entry<M, NOP>(vs[u], xs[u], s);
            } else {
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    if (e + u < n) {
                        const long long c = col[64LL * (e + u)];
                        double xs[M], vs[NOP];
                        krylov_load_point<M>(in + c * M, xs);
#pragma unroll
                        for (int o = 0; o < NOP; ++o) vs[o] = val[o * q.total + 64LL * (e + u)];
                        krylov_point_entry<M, NOP>(vs, xs, s);
                    }
                }
            }
        }
        if (row < q.npoints) {
            const double* cp = q.cpt + row;
            double t[M];
#pragma unroll
            for (int a = 0; a < M; ++a) {
                t[a] = cp[(long long)(a * M * NOP) * q.npoints] * s[0][0];
#pragma unroll
                for (int b = 0; b < M; ++b) {
#pragma unroll
                    for (int o = 0; o < NOP; ++o) {
                        if (b + o > 0) t[a] = __builtin_fma(cp[(long long)((a * M + b) * NOP + o) * q.npoints], s[o][b], t[a]);
                    }
                }
            }
            krylov_system_finish<M>(q, mode, in, w, out, out2, row, t, pa, pb);
        }
    }
    block_sums<true>(pa, pb, partial, gridDim.x);
}

// dinv[i * m + a] = 1 / (D_aa,i + sum_o c[a][a][o][i] own_o): krylov_system_diag_kernel's sums and count with the point's own coefficients.
// On the transposed arrays the own entries of row i are the same numbers, so M^T takes the same kernel there.
template <int M, int NOP>
__global__ void __launch_bounds__(256) krylov_system_diag_point_kernel(const KrylovCoupled q, double* dinv, double* partial) {
    const int lane = threadIdx.x & 63;
    const long long sl = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long row = sl * 64 + lane;
    double bad = 0.0;
    if (sl * 64 < q.npoints) {                                   // wave-uniform
        const int wid = __builtin_amdgcn_readfirstlane(q.width[sl]);
        const long long at = q.soff[sl] + lane;
        int n = row < q.npoints ? q.len[row] : 0;
        n = n < wid ? n : wid;
        double own[NOP];
#pragma unroll
        for (int o = 0; o < NOP; ++o) own[o] = 0.0;
        for (int e = 0; e < wid; ++e) {                          // wave-uniform
            if (e < n && q.col[at + 64LL * e] == row) {
#pragma unroll
                for (int o = 0; o < NOP; ++o) own[o] += q.val[o * q.total + at + 64LL * e];
            }
        }
        if (row < q.npoints) {
            const double* cp = q.cpt + row;
            bool unusable = false;
#pragma unroll
            for (int a = 0; a < M; ++a) {
                double t = cp[(long long)((a * M + a) * NOP) * q.npoints] * own[0];
#pragma unroll
                for (int o = 1; o < NOP; ++o) t = t + cp[(long long)((a * M + a) * NOP + o) * q.npoints] * own[o];
                const double diag = (q.dten ? q.dten[(a * M + a) * q.npoints + row] : q.dconst[a * M + a]) + t;
                const bool ok = diag != 0.0 && __builtin_isfinite(diag);
                dinv[row * M + a] = ok ? 1.0 / diag : 0.0;
                unusable = unusable || !ok;
            }
            bad = unusable ? 1.0 : 0.0;
        }
    }
    block_sums<false>(bad, 0.0, partial, gridDim.x);
}

// z[i][o][b] = sum_a c[a][b][o][i] in[i][a]: pointwise, every coefficient one coalesced run.
template <int M, int NOP>
__global__ void __launch_bounds__(256) krylov_system_mix_kernel(const KrylovCoupled q, int mode, const double* in, double* z, const KrylovScalars* sc) {
    if (mode != SYSTEM_PRODUCT && sc->done) return;              // uniform: the whole grid
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= q.npoints) return;
    double li[M];
    krylov_load_point<M>(in + i * M, li);
    const double* cp = q.cpt + i;
    double* zi = z + i * (NOP * M);
#pragma unroll
    for (int o = 0; o < NOP; ++o) {
#pragma unroll
        for (int b = 0; b < M; ++b) {
            double t = cp[(long long)(b * NOP + o) * q.npoints] * li[0];
#pragma unroll
            for (int a = 1; a < M; ++a) t = __builtin_fma(cp[(long long)((a * M + b) * NOP + o) * q.npoints], li[a], t);
            zi[o * M + b] = t;
        }
    }
}

template <int M, int NOP>
__device__ __forceinline__ void krylov_mixed_entry(const double (&vs)[NOP], const double (&zs)[NOP * M], double (&acc)[M]) {
#pragma unroll
    for (int o = 0; o < NOP; ++o) {
#pragma unroll
        for (int b = 0; b < M; ++b) acc[b] = __builtin_fma(vs[o], zs[o * M + b], acc[b]);
    }
}

// y = M^T in from z = mix(in): q holds the operator's transposed arrays and dswap = 1.
template <int M, int NOP>
__global__ void __launch_bounds__(256) krylov_system_spmv_mixed_kernel(const KrylovCoupled q, int mode, const double* in, const double* z,
                                                                       const double* w, double* out, double* out2, double* partial,
                                                                       const KrylovScalars* sc) {
    if (mode != SYSTEM_PRODUCT && sc->done) return;              // uniform: the whole grid
    constexpr int UNROLL = M * NOP > 16 ? 2 : 4;
    const int lane = threadIdx.x & 63;
    const long long sl = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long row = sl * 64 + lane;
    double pa = 0.0, pb = 0.0;
    if (sl * 64 < q.npoints) {                                   // wave-uniform
        const int wid = __builtin_amdgcn_readfirstlane(q.width[sl]);
        const long long at = q.soff[sl] + lane;
        int n = row < q.npoints ? q.len[row] : 0;
        n = n < wid ? n : wid;
        const int32_t* col = q.col + at;
        const double* val = q.val + at;
        double acc[M];
#pragma unroll
        for (int b = 0; b < M; ++b) acc[b] = 0.0;
        for (int e = 0; e < wid; e += UNROLL) {                  // wave-uniform
            if (e + UNROLL <= n) {
                double zs[UNROLL][NOP * M], vs[UNROLL][NOP];
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    const long long c = col[64LL * (e + u)];
                    krylov_load_point<NOP * M>(z + c * (NOP * M), zs[u]);
#pragma unroll
                    for (int o = 0; o < NOP; ++o) vs[u][o] = val[o * q.total + 64LL * (e + u)];
                }
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) krylov_mixed_entry<M, NOP>(vs[u], zs[u], acc);
            } else {
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    if (e + u < n) {
                        const long long c = col[64LL * (e + u)];
                        double zs[NOP * M], vs[NOP];
                        krylov_load_point<NOP * M>(z + c * (NOP * M), zs);
#pragma unroll
                        for (int o = 0; o < NOP; ++o) vs[o] = val[o * q.total + 64LL * (e + u)];
                        krylov_mixed_entry<M, NOP>(vs, zs, acc);
                    }
                }
            }
        }
        if (row < q.npoints) krylov_system_finish<M>(q, mode, in, w, out, out2, row, acc, pa, pb);
    }
    block_sums<true>(pa, pb, partial, gridDim.x);
}

struct KrylovPointCall {
    KrylovSystemCall c;
    double* mixed;                                              // z, nop m npoints doubles: the transposed calls only
};

template <int M, int NOP>
static void krylov_point_product(const KrylovPointCall& p, int mode, const double* in, const double* w, double* out, double* out2) {
    const KrylovSystemCall& c = p.c;
    const dim3 pgrid((unsigned)((c.q.npoints + 255) / 256)), block(256);
    if (c.q.dswap) {
        hipLaunchKernelGGL((krylov_system_mix_kernel<M, NOP>), pgrid, block, 0, c.s, c.q, mode, in, p.mixed, (const KrylovScalars*)c.w.sc);
        hipLaunchKernelGGL((krylov_system_spmv_mixed_kernel<M, NOP>), pgrid, block, 0, c.s, c.q, mode, in, (const double*)p.mixed, w, out, out2,
                           c.w.partial, (const KrylovScalars*)c.w.sc);
    } else {
        hipLaunchKernelGGL((krylov_system_spmv_point_kernel<M, NOP>), pgrid, block, 0, c.s, c.q, mode, in, w, out, out2, c.w.partial,
                           (const KrylovScalars*)c.w.sc);
    }
}

// krylov_system_run's launch lists with the per-point products: 8 launches per forward iteration, 10 per transposed one.
template <int M, int NOP>
static void krylov_point_run(const KrylovPointCall& p) {
    const KrylovSystemCall& c = p.c;
    const KrylovWork& w = c.w;
    const long long nwgp = (c.q.npoints + 255) / 256, nrows = c.q.npoints * M;
    const dim3 pgrid((unsigned)nwgp), ugrid((unsigned)w.nwg), block(256);
    const KrylovScalars* sc = w.sc;
    hipStream_t s = c.s;
    double* const none = nullptr;
    const char* product = c.q.dswap ? "krylov-system-spmv-mixed" : "krylov-system-spmv-point";
    if (c.what == SYSTEM_CALL_START) {
        if (c.W) {
            krylov_system_block_counts(c.q.npoints, M, c.points, w, c.W, c.rtol, c.atol, c.maxiter, s);
        } else {
            if (c.jacobi) {
                hipLaunchKernelGGL((krylov_system_diag_point_kernel<M, NOP>), pgrid, block, 0, s, c.q, w.dinv, w.partial);
                note_kernel("krylov-system-diag-point");
            }
            krylov_reduce(REDUCE_DIAG, w, c.jacobi ? nwgp : 0, 1, c.rtol, c.atol, c.maxiter, s);
        }
        krylov_point_product<M, NOP>(p, SYSTEM_RESIDUAL, c.in, c.other, w.r, w.r0);
        note_kernel(product);
        krylov_reduce(REDUCE_RESIDUAL, w, nwgp, 2, c.rtol, c.atol, c.maxiter, s);
        note_kernel("krylov-reduce");
    } else if (c.what == SYSTEM_CALL_ITERATE) {
        for (int64_t it = 0; it < c.niter; ++it) {
            if (c.W) krylov_system_update_block<UPDATE_P>(c.q.npoints, M, c.points, w, c.W, s);
            else hipLaunchKernelGGL((krylov_update_kernel<UPDATE_P>), ugrid, block, 0, s, nrows, w, c.x, sc);
            krylov_point_product<M, NOP>(p, SYSTEM_V, w.phat, w.r0, w.v, none);
            krylov_reduce(REDUCE_ALPHA, w, nwgp, 1, 0.0, 0.0, 0, s);
            if (c.W) krylov_system_update_block<UPDATE_S>(c.q.npoints, M, c.points, w, c.W, s);
            else hipLaunchKernelGGL((krylov_update_kernel<UPDATE_S>), ugrid, block, 0, s, nrows, w, c.x, sc);
            krylov_point_product<M, NOP>(p, SYSTEM_T, w.shat, w.s, w.t, none);
            krylov_reduce(REDUCE_OMEGA, w, nwgp, 2, 0.0, 0.0, 0, s);
            hipLaunchKernelGGL((krylov_update_kernel<UPDATE_X>), ugrid, block, 0, s, nrows, w, c.x, sc);
            krylov_reduce(REDUCE_RHO, w, w.nwg, 2, 0.0, 0.0, 0, s);
        }
        note_kernel(c.W ? "krylov-system-update-block" : "krylov-update");
    } else {
        krylov_point_product<M, NOP>(p, SYSTEM_PRODUCT, c.in, c.other, c.x, none);
        krylov_reduce(REDUCE_PRODUCT, w, nwgp, 2, 0.0, 0.0, 0, s);
        note_kernel(product);
    }
}

template <int M>
static void krylov_point_planes(int nop, const KrylovPointCall& p) {
    switch (nop) {
    case 1: krylov_point_run<M, 1>(p); break;
    case 2: krylov_point_run<M, 2>(p); break;
    case 3: krylov_point_run<M, 3>(p); break;
    case 4: krylov_point_run<M, 4>(p); break;
    case 5: krylov_point_run<M, 5>(p); break;
    case 6: krylov_point_run<M, 6>(p); break;
    case 7: krylov_point_run<M, 7>(p); break;
    default: krylov_point_run<M, 8>(p); break;
    }
}

// krylov_system_call for a per-point table: its checks, then those of the tensor and of z, then the call's launches.
static int krylov_point_call(const char* who, KrylovPointCall& p, int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                             const int64_t* soff, const int32_t* col, const double* val, int64_t total, int nop, int m,
                             const double* coupling, const double* diag, const double* diag_const, int transposed, void* workspace,
                             int device) {
    const std::string name(who);
    KrylovSystemCall& c = p.c;
    if (m < 1 || m > KRYLOV_SYSTEM_FIELDS) { set_error(name + ": m must be 1 .. 4"); return WLSQM_EVALUE; }
    if (nop < 1 || nop > KRYLOV_SYSTEM_PLANES) { set_error(name + ": nop must be 1 .. 8"); return WLSQM_EVALUE; }
    if (npoints < 1 || nslices < 0 || npoints > 64 * nslices || total < 0 || (npoints * m + 255) / 256 > 0x7fffffffLL) {
        set_error(name + ": npoints must be 1 .. 64 * nslices");
        return WLSQM_EVALUE;
    }
    if (!len || !width || !soff || !col || !val || !coupling || !workspace || (!diag && !diag_const) || !c.in || !c.other || !c.x
        || (transposed && !p.mixed)) {
        set_error(name + ": null array");
        return WLSQM_EVALUE;
    }
    if (m % 2 == 0 && (((uintptr_t)c.in | (uintptr_t)c.other | (uintptr_t)c.x | (uintptr_t)workspace) & 15)) {
        set_error(name + ": with m = 2 or 4 the vectors and the workspace must be 16-byte aligned");
        return WLSQM_EVALUE;
    }
    if (((uintptr_t)coupling & 7) || (transposed && ((uintptr_t)p.mixed & 15))) {
        set_error(name + ": coupling must be 8-byte aligned and the mixed plane 16-byte aligned");
        return WLSQM_EVALUE;
    }
    KrylovCoupled& q = c.q;
    q.npoints = npoints; q.total = total;
    q.len = len; q.width = width; q.soff = reinterpret_cast<const long long*>(soff);
    q.col = col; q.val = val; q.dten = diag; q.dswap = transposed ? 1 : 0; q.cpt = coupling;
    for (int i = 0; i < KRYLOV_SYSTEM_FIELDS * KRYLOV_SYSTEM_FIELDS; ++i) q.dconst[i] = 0.0;
    for (int a = 0; a < m && !diag; ++a) {                      // block (a, b) of M^T takes D_ba
        for (int b = 0; b < m; ++b) q.dconst[a * m + b] = transposed ? diag_const[b * m + a] : diag_const[a * m + b];
    }
    for (int i = 0; i < KRYLOV_SYSTEM_FIELDS * KRYLOV_SYSTEM_FIELDS * KRYLOV_SYSTEM_PLANES; ++i) q.coupling[i] = 0.0;
    DeviceScope scope;
    const int rc = scope.enter(device);
    if (rc != WLSQM_OK) return rc;
    c.w = krylov_work(workspace, npoints * m, c.jacobi != 0);
    switch (m) {
    case 1: krylov_point_planes<1>(nop, p); break;
    case 2: krylov_point_planes<2>(nop, p); break;
    case 3: krylov_point_planes<3>(nop, p); break;
    default: krylov_point_planes<4>(nop, p); break;
    }
    WLSQM_HIP_CHECK(hipGetLastError());
    return WLSQM_OK;
}

// wlsqm_hip_krylov_system_grads_device and its per-point form: `coupling` is the host table, or the device tensor when `point`.
static int krylov_system_grads_call(const char* who, bool point, int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                    const int64_t* soff, const int32_t* col, int64_t total, int nop, int m, const double* coupling,
                                    const double* lam, const double* x, double* grad_val, double* grad_diag, int device, void* stream) {
    const std::string name(who);
    if (m < 1 || m > KRYLOV_SYSTEM_FIELDS) { set_error(name + ": m must be 1 .. 4"); return WLSQM_EVALUE; }
    if (nop < 1 || nop > KRYLOV_SYSTEM_PLANES) { set_error(name + ": nop must be 1 .. 8"); return WLSQM_EVALUE; }
    if (npoints < 1 || nslices < 0 || npoints > 64 * nslices || total < 0 || (npoints + 255) / 256 > 0x7fffffffLL) {
        set_error(name + ": npoints must be 1 .. 64 * nslices");
        return WLSQM_EVALUE;
    }
    if (!len || !width || !soff || !col || !coupling || !lam || !x) { set_error(name + ": null array"); return WLSQM_EVALUE; }
    if (total == 0) grad_val = nullptr;                          // no stored entry: nothing to write
    if (!grad_val && !grad_diag) {
        if (total == 0) return WLSQM_OK;
        set_error(name + ": no output is asked for");
        return WLSQM_EVALUE;
    }
    if (m % 2 == 0 && (((uintptr_t)lam | (uintptr_t)x) & 15)) {
        set_error(name + ": with m = 2 or 4 lam and x must be 16-byte aligned");
        return WLSQM_EVALUE;
    }
    if (point && ((uintptr_t)coupling & 7)) { set_error(name + ": coupling must be 8-byte aligned"); return WLSQM_EVALUE; }
    KrylovCoupled q;
    q.npoints = npoints; q.total = total;
    q.len = len; q.width = width; q.soff = reinterpret_cast<const long long*>(soff);
    q.col = col; q.val = nullptr; q.dten = nullptr; q.dswap = 0; q.cpt = point ? coupling : nullptr;
    for (int i = 0; i < KRYLOV_SYSTEM_FIELDS * KRYLOV_SYSTEM_FIELDS; ++i) q.dconst[i] = 0.0;
    for (int i = 0; i < KRYLOV_SYSTEM_FIELDS * KRYLOV_SYSTEM_FIELDS * KRYLOV_SYSTEM_PLANES; ++i) q.coupling[i] = (!point && i < m * m * nop) ? coupling[i] : 0.0;
    DeviceScope scope;
    const int rc = scope.enter(device);
    if (rc != WLSQM_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    switch (m) {
    case 1: krylov_system_grads_planes<1>(nop, q, lam, x, grad_val, grad_diag, s); break;
    case 2: krylov_system_grads_planes<2>(nop, q, lam, x, grad_val, grad_diag, s); break;
    case 3: krylov_system_grads_planes<3>(nop, q, lam, x, grad_val, grad_diag, s); break;
    default: krylov_system_grads_planes<4>(nop, q, lam, x, grad_val, grad_diag, s); break;
    }
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("krylov-system-grads");
    return WLSQM_OK;
}

}  // namespace wlsqm

using namespace wlsqm;

extern "C" {

int64_t wlsqm_hip_krylov_workspace_bytes(int64_t nrows) {
    if (nrows < 0) return -1;
    return (int64_t)sizeof(double) * (KRYLOV_HEAD + 2 * ((nrows + 255) / 256) + KRYLOV_VECTORS * nrows);
}

int wlsqm_hip_krylov_start_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                  const int32_t* col, const double* val, const double* diag, double diag_const, double scale, int jacobi,
                                  const double* b, const double* x, double rtol, double atol, int64_t maxiter, void* workspace,
                                  int device, void* stream) {
    KrylovSys m;
    int rc = krylov_system("krylov_start", m, nrows, nslices, len, width, soff, col, val, diag, diag_const, scale, workspace);
    if (rc != WLSQM_OK) return rc;
    if (!b || !x) { set_error("krylov_start: null array"); return WLSQM_EVALUE; }
    if (!(rtol >= 0.0) || !(atol >= 0.0) || !std::isfinite(rtol) || !std::isfinite(atol)) {
        set_error("krylov_start: rtol and atol must be finite and >= 0");
        return WLSQM_EVALUE;
    }
    if (maxiter < 0 || maxiter > INT32_MAX) { set_error("krylov_start: maxiter must be 0 .. 2^31 - 1"); return WLSQM_EVALUE; }
    DeviceScope scope;
    rc = scope.enter(device);
    if (rc != WLSQM_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const KrylovWork w = krylov_work(workspace, nrows, jacobi != 0);
    const dim3 grid((unsigned)w.nwg);
    if (jacobi) {
        hipLaunchKernelGGL(krylov_diag_kernel, grid, dim3(256), 0, s, m, w.dinv, w.partial);
        note_kernel("krylov-diag");
    }
    krylov_reduce(REDUCE_DIAG, w, jacobi ? w.nwg : 0, 1, rtol, atol, (int)maxiter, s);
    hipLaunchKernelGGL((krylov_spmv_kernel<SPMV_RESIDUAL>), grid, dim3(256), 0, s, m, x, b, w.r, w.r0, w.partial, (const KrylovScalars*)w.sc, 0);
    note_kernel("krylov-spmv-dot");
    krylov_reduce(REDUCE_RESIDUAL, w, w.nwg, 2, rtol, atol, (int)maxiter, s);
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("krylov-reduce");
    return WLSQM_OK;
}

int wlsqm_hip_krylov_bicgstab_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                     const int32_t* col, const double* val, const double* diag, double diag_const, double scale, int jacobi,
                                     double* x, int64_t niter, void* workspace, int device, void* stream) {
    KrylovSys m;
    int rc = krylov_system("krylov_bicgstab", m, nrows, nslices, len, width, soff, col, val, diag, diag_const, scale, workspace);
    if (rc != WLSQM_OK) return rc;
    if (!x) { set_error("krylov_bicgstab: null array"); return WLSQM_EVALUE; }
    if (niter < 0) { set_error("krylov_bicgstab: niter must be >= 0"); return WLSQM_EVALUE; }
    DeviceScope scope;
    rc = scope.enter(device);
    if (rc != WLSQM_OK || niter == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    const KrylovWork w = krylov_work(workspace, nrows, jacobi != 0);
    const dim3 grid((unsigned)w.nwg);
    const KrylovScalars* sc = w.sc;
    for (int64_t it = 0; it < niter; ++it) {
        hipLaunchKernelGGL((krylov_update_kernel<UPDATE_P>), grid, dim3(256), 0, s, (long long)nrows, w, x, sc);
        hipLaunchKernelGGL((krylov_spmv_kernel<SPMV_V>), grid, dim3(256), 0, s, m, (const double*)w.phat, (const double*)w.r0, w.v, (double*)nullptr, w.partial, sc, 0);
        krylov_reduce(REDUCE_ALPHA, w, w.nwg, 1, 0.0, 0.0, 0, s);
        hipLaunchKernelGGL((krylov_update_kernel<UPDATE_S>), grid, dim3(256), 0, s, (long long)nrows, w, x, sc);
        hipLaunchKernelGGL((krylov_spmv_kernel<SPMV_T>), grid, dim3(256), 0, s, m, (const double*)w.shat, (const double*)w.s, w.t, (double*)nullptr, w.partial, sc, 0);
        krylov_reduce(REDUCE_OMEGA, w, w.nwg, 2, 0.0, 0.0, 0, s);
        hipLaunchKernelGGL((krylov_update_kernel<UPDATE_X>), grid, dim3(256), 0, s, (long long)nrows, w, x, sc);
        krylov_reduce(REDUCE_RHO, w, w.nwg, 2, 0.0, 0.0, 0, s);
    }
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("krylov-update");
    return WLSQM_OK;
}

int wlsqm_hip_krylov_product_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                    const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                    const double* in, const double* w, double* out, void* workspace, int device, void* stream) {
    KrylovSys m;
    int rc = krylov_system("krylov_product", m, nrows, nslices, len, width, soff, col, val, diag, diag_const, scale, workspace);
    if (rc != WLSQM_OK) return rc;
    if (!in || !w || !out) { set_error("krylov_product: null array"); return WLSQM_EVALUE; }
    DeviceScope scope;
    rc = scope.enter(device);
    if (rc != WLSQM_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const KrylovWork k = krylov_work(workspace, nrows, false);
    hipLaunchKernelGGL((krylov_spmv_kernel<SPMV_T>), dim3((unsigned)k.nwg), dim3(256), 0, s, m, in, w, out, (double*)nullptr, k.partial,
                       (const KrylovScalars*)k.sc, 1);
    krylov_reduce(REDUCE_PRODUCT, k, k.nwg, 2, 0.0, 0.0, 0, s);
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("krylov-spmv-dot");
    return WLSQM_OK;
}

int wlsqm_hip_krylov_grads_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                  const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                  const double* lam, const double* x, double* grad_val, double* grad_diag, int want_scale,
                                  void* workspace, int device, void* stream) {
    KrylovSys m;
    int rc = krylov_system("krylov_grads", m, nrows, nslices, len, width, soff, col, val, diag, diag_const, scale, workspace);
    if (rc != WLSQM_OK) return rc;
    if (!lam || !x) { set_error("krylov_grads: null array"); return WLSQM_EVALUE; }
    if (!grad_val && !grad_diag && !want_scale) { set_error("krylov_grads: no output is asked for"); return WLSQM_EVALUE; }
    DeviceScope scope;
    rc = scope.enter(device);
    if (rc != WLSQM_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const KrylovWork k = krylov_work(workspace, nrows, false);
    switch ((grad_val ? 4 : 0) | (grad_diag ? 2 : 0) | (want_scale ? 1 : 0)) {
    case 1: krylov_grads_launch<false, false, true>(m, k, lam, x, grad_val, grad_diag, s); break;
    case 2: krylov_grads_launch<false, true, false>(m, k, lam, x, grad_val, grad_diag, s); break;
    case 3: krylov_grads_launch<false, true, true>(m, k, lam, x, grad_val, grad_diag, s); break;
    case 4: krylov_grads_launch<true, false, false>(m, k, lam, x, grad_val, grad_diag, s); break;
    case 5: krylov_grads_launch<true, false, true>(m, k, lam, x, grad_val, grad_diag, s); break;
    case 6: krylov_grads_launch<true, true, false>(m, k, lam, x, grad_val, grad_diag, s); break;
    default: krylov_grads_launch<true, true, true>(m, k, lam, x, grad_val, grad_diag, s); break;
    }
    if (want_scale) krylov_reduce(REDUCE_NEGATED, k, k.nwg, 1, 0.0, 0.0, 0, s);
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("krylov-grads");
    return WLSQM_OK;
}

int64_t wlsqm_hip_krylov_block_bytes(int64_t nrows, int block) {
    if (nrows < 0 || (block != 8 && block != 16 && block != 32)) return -1;
    return (int64_t)sizeof(double) * (krylov_plane_doubles((nrows + 63) / 64, block) + (nrows + 255) / 256);
}

int wlsqm_hip_krylov_block_factor_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                         const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                         int block, void* planes, void* planes_t, int device, void* stream) {
    KrylovSys m;
    int rc = krylov_block_size("krylov_block_factor", block, planes);
    if (rc != WLSQM_OK) return rc;
    rc = krylov_system("krylov_block_factor", m, nrows, nslices, len, width, soff, col, val, diag, diag_const, scale, planes);
    if (rc != WLSQM_OK) return rc;
    if (nslices != (nrows + 63) / 64) { set_error("krylov_block_factor: nslices must be ceil(nrows / 64)"); return WLSQM_EVALUE; }
    DeviceScope scope;
    rc = scope.enter(device);
    if (rc != WLSQM_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((nrows + 255) / 256));
    double *W = static_cast<double*>(planes), *WT = static_cast<double*>(planes_t);
    switch (block) {
    case 8: hipLaunchKernelGGL(krylov_blocks_kernel<8>, grid, dim3(256), 0, s, m, (long long)nslices, W, WT); break;
    case 16: hipLaunchKernelGGL(krylov_blocks_kernel<16>, grid, dim3(256), 0, s, m, (long long)nslices, W, WT); break;
    default: hipLaunchKernelGGL(krylov_blocks_kernel<32>, grid, dim3(256), 0, s, m, (long long)nslices, W, WT); break;
    }
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("krylov-blocks");
    return WLSQM_OK;
}

int wlsqm_hip_krylov_block_start_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                        const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                        int block, const void* planes, const double* b, const double* x, double rtol, double atol,
                                        int64_t maxiter, void* workspace, int device, void* stream) {
    KrylovSys m;
    int rc = krylov_block_size("krylov_block_start", block, planes);
    if (rc != WLSQM_OK) return rc;
    rc = krylov_system("krylov_block_start", m, nrows, nslices, len, width, soff, col, val, diag, diag_const, scale, workspace);
    if (rc != WLSQM_OK) return rc;
    if (nslices != (nrows + 63) / 64) { set_error("krylov_block_start: nslices must be ceil(nrows / 64)"); return WLSQM_EVALUE; }
    if (!b || !x) { set_error("krylov_block_start: null array"); return WLSQM_EVALUE; }
    if (!(rtol >= 0.0) || !(atol >= 0.0) || !std::isfinite(rtol) || !std::isfinite(atol)) {
        set_error("krylov_block_start: rtol and atol must be finite and >= 0");
        return WLSQM_EVALUE;
    }
    if (maxiter < 0 || maxiter > INT32_MAX) { set_error("krylov_block_start: maxiter must be 0 .. 2^31 - 1"); return WLSQM_EVALUE; }
    DeviceScope scope;
    rc = scope.enter(device);
    if (rc != WLSQM_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const KrylovWork w = krylov_work(workspace, nrows, true);
    const dim3 grid((unsigned)w.nwg);
    const double* counts = static_cast<const double*>(planes) + krylov_plane_doubles(nslices, block);
    hipLaunchKernelGGL(krylov_reduce_kernel, dim3(1), dim3(256), 0, s, (int)REDUCE_DIAG, counts, w.nwg, 1, w.sc, rtol, atol, (int)maxiter);
    hipLaunchKernelGGL((krylov_spmv_kernel<SPMV_RESIDUAL>), grid, dim3(256), 0, s, m, x, b, w.r, w.r0, w.partial, (const KrylovScalars*)w.sc, 0);
    note_kernel("krylov-spmv-dot");
    krylov_reduce(REDUCE_RESIDUAL, w, w.nwg, 2, rtol, atol, (int)maxiter, s);
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("krylov-reduce");
    return WLSQM_OK;
}

int wlsqm_hip_krylov_block_bicgstab_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                           const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                           int block, const void* planes, double* x, int64_t niter, void* workspace, int device,
                                           void* stream) {
    KrylovSys m;
    int rc = krylov_block_size("krylov_block_bicgstab", block, planes);
    if (rc != WLSQM_OK) return rc;
    rc = krylov_system("krylov_block_bicgstab", m, nrows, nslices, len, width, soff, col, val, diag, diag_const, scale, workspace);
    if (rc != WLSQM_OK) return rc;
    if (nslices != (nrows + 63) / 64) { set_error("krylov_block_bicgstab: nslices must be ceil(nrows / 64)"); return WLSQM_EVALUE; }
    if (!x) { set_error("krylov_block_bicgstab: null array"); return WLSQM_EVALUE; }
    if (niter < 0) { set_error("krylov_block_bicgstab: niter must be >= 0"); return WLSQM_EVALUE; }
    DeviceScope scope;
    rc = scope.enter(device);
    if (rc != WLSQM_OK || niter == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    const KrylovWork w = krylov_work(workspace, nrows, true);
    const double* W = static_cast<const double*>(planes);
    switch (block) {
    case 8: krylov_block_iterations<8>(m, w, W, x, niter, s); break;
    case 16: krylov_block_iterations<16>(m, w, W, x, niter, s); break;
    default: krylov_block_iterations<32>(m, w, W, x, niter, s); break;
    }
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("krylov-update-block");
    return WLSQM_OK;
}

int wlsqm_hip_krylov_block_precondition_device(int64_t nrows, int block, const void* planes, const double* v, double* out, int device,
                                               void* stream) {
    int rc = krylov_block_size("krylov_block_precondition", block, planes);
    if (rc != WLSQM_OK) return rc;
    if (nrows < 1 || (nrows + 255) / 256 > 0x7fffffffLL) { set_error("krylov_block_precondition: nrows must be >= 1"); return WLSQM_EVALUE; }
    if (!v || !out) { set_error("krylov_block_precondition: null array"); return WLSQM_EVALUE; }
    DeviceScope scope;
    rc = scope.enter(device);
    if (rc != WLSQM_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((nrows + 255) / 256));
    const double* W = static_cast<const double*>(planes);
    switch (block) {
    case 8: hipLaunchKernelGGL(krylov_precondition_kernel<8>, grid, dim3(256), 0, s, (long long)nrows, W, v, out); break;
    case 16: hipLaunchKernelGGL(krylov_precondition_kernel<16>, grid, dim3(256), 0, s, (long long)nrows, W, v, out); break;
    default: hipLaunchKernelGGL(krylov_precondition_kernel<32>, grid, dim3(256), 0, s, (long long)nrows, W, v, out); break;
    }
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("krylov-precondition");
    return WLSQM_OK;
}

int64_t wlsqm_hip_krylov_many_workspace_bytes(int64_t nrows, int nfields) {
    if (nrows < 0 || nfields < 1 || nfields > KRYLOV_MANY_FIELDS) return -1;
    const int pitch = krylov_pitch(nfields);
    return (int64_t)sizeof(double) * (KRYLOV_MANY_HEAD + krylov_many_partials((nrows + 255) / 256, pitch)
                                      + (int64_t)KRYLOV_MANY_VECTORS * pitch * nrows + nrows);
}

int wlsqm_hip_krylov_many_start_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                       const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                       int nfields, const double* b, int64_t b_stride_field, int64_t b_stride_point, const double* x,
                                       int64_t x_stride_field, int64_t x_stride_point, int precond, const void* planes, double rtol,
                                       double atol, int64_t maxiter, void* workspace, int device, void* stream) {
    KrylovSys m;
    int rc = krylov_system("krylov_many_start", m, nrows, nslices, len, width, soff, col, val, diag, diag_const, scale, workspace);
    if (rc != WLSQM_OK) return rc;
    rc = krylov_many_arguments("krylov_many_start", nrows, nslices, nfields, precond, planes, workspace);
    if (rc != WLSQM_OK) return rc;
    if (!b || !x) { set_error("krylov_many_start: null array"); return WLSQM_EVALUE; }
    if (!(rtol >= 0.0) || !(atol >= 0.0) || !std::isfinite(rtol) || !std::isfinite(atol)) {
        set_error("krylov_many_start: rtol and atol must be finite and >= 0");
        return WLSQM_EVALUE;
    }
    if (maxiter < 0 || maxiter > INT32_MAX) { set_error("krylov_many_start: maxiter must be 0 .. 2^31 - 1"); return WLSQM_EVALUE; }
    DeviceScope scope;
    rc = scope.enter(device);
    if (rc != WLSQM_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int pitch = krylov_pitch(nfields);
    const KrylovManyWork w = krylov_many_work(workspace, nrows, pitch, precond != 0);
    const KrylovFields bf{const_cast<double*>(b), b_stride_field, b_stride_point}, xf{const_cast<double*>(x), x_stride_field, x_stride_point};
    switch (pitch) {
    case 2: krylov_many_start<2>(m, w, nfields, bf, xf, precond, planes, nslices, rtol, atol, (int)maxiter, s); break;
    case 4: krylov_many_start<4>(m, w, nfields, bf, xf, precond, planes, nslices, rtol, atol, (int)maxiter, s); break;
    default: krylov_many_start<8>(m, w, nfields, bf, xf, precond, planes, nslices, rtol, atol, (int)maxiter, s); break;
    }
    WLSQM_HIP_CHECK(hipGetLastError());
    return WLSQM_OK;
}

int wlsqm_hip_krylov_many_bicgstab_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                          const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                          int nfields, double* x, int64_t x_stride_field, int64_t x_stride_point, int precond,
                                          const void* planes, int64_t niter, void* workspace, int device, void* stream) {
    KrylovSys m;
    int rc = krylov_system("krylov_many_bicgstab", m, nrows, nslices, len, width, soff, col, val, diag, diag_const, scale, workspace);
    if (rc != WLSQM_OK) return rc;
    rc = krylov_many_arguments("krylov_many_bicgstab", nrows, nslices, nfields, precond, planes, workspace);
    if (rc != WLSQM_OK) return rc;
    if (!x) { set_error("krylov_many_bicgstab: null array"); return WLSQM_EVALUE; }
    if (niter < 0) { set_error("krylov_many_bicgstab: niter must be >= 0"); return WLSQM_EVALUE; }
    DeviceScope scope;
    rc = scope.enter(device);
    if (rc != WLSQM_OK || niter == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int pitch = krylov_pitch(nfields);
    const KrylovManyWork w = krylov_many_work(workspace, nrows, pitch, precond != 0);
    const KrylovFields xf{x, x_stride_field, x_stride_point};
    switch (pitch) {
    case 2: krylov_many_iterate<2>(m, w, nfields, xf, precond, planes, niter, s); break;
    case 4: krylov_many_iterate<4>(m, w, nfields, xf, precond, planes, niter, s); break;
    default: krylov_many_iterate<8>(m, w, nfields, xf, precond, planes, niter, s); break;
    }
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel(precond > 1 ? "krylov-update-block-many" : "krylov-update-many");
    return WLSQM_OK;
}

int wlsqm_hip_krylov_many_product_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                         const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                         int nfields, const double* in, int64_t in_stride_field, int64_t in_stride_point, const double* w,
                                         int64_t w_stride_field, int64_t w_stride_point, double* out, int64_t out_stride_field,
                                         int64_t out_stride_point, void* workspace, int device, void* stream) {
    KrylovSys m;
    int rc = krylov_system("krylov_many_product", m, nrows, nslices, len, width, soff, col, val, diag, diag_const, scale, workspace);
    if (rc != WLSQM_OK) return rc;
    rc = krylov_many_arguments("krylov_many_product", nrows, nslices, nfields, 0, nullptr, workspace);
    if (rc != WLSQM_OK) return rc;
    if (!in || !w || !out) { set_error("krylov_many_product: null array"); return WLSQM_EVALUE; }
    DeviceScope scope;
    rc = scope.enter(device);
    if (rc != WLSQM_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int pitch = krylov_pitch(nfields);
    const KrylovManyWork k = krylov_many_work(workspace, nrows, pitch, false);
    const KrylovFields inf{const_cast<double*>(in), in_stride_field, in_stride_point}, wf{const_cast<double*>(w), w_stride_field, w_stride_point},
        outf{out, out_stride_field, out_stride_point};
    switch (pitch) {
    case 2: krylov_many_product<2>(m, k, nfields, inf, wf, outf, s); break;
    case 4: krylov_many_product<4>(m, k, nfields, inf, wf, outf, s); break;
    default: krylov_many_product<8>(m, k, nfields, inf, wf, outf, s); break;
    }
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("krylov-spmv-many");
    return WLSQM_OK;
}

int64_t wlsqm_hip_krylov_l2_workspace_bytes(int64_t nrows) {
    if (nrows < 0) return -1;
    return (int64_t)sizeof(double) * (KRYLOV_HEAD + KRYLOV_L2_PLANES * ((nrows + 255) / 256) + KRYLOV_L2_VECTORS * nrows);
}

int wlsqm_hip_krylov_l2_start_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                     const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                     int precond, const void* planes, const double* b, const double* x, double rtol, double atol,
                                     int64_t maxiter, void* workspace, int device, void* stream) {
    KrylovSys m;
    int rc = krylov_system("krylov_l2_start", m, nrows, nslices, len, width, soff, col, val, diag, diag_const, scale, workspace);
    if (rc != WLSQM_OK) return rc;
    rc = krylov_many_arguments("krylov_l2_start", nrows, nslices, 1, precond, planes, workspace);
    if (rc != WLSQM_OK) return rc;
    if (!b || !x) { set_error("krylov_l2_start: null array"); return WLSQM_EVALUE; }
    if (!(rtol >= 0.0) || !(atol >= 0.0) || !std::isfinite(rtol) || !std::isfinite(atol)) {
        set_error("krylov_l2_start: rtol and atol must be finite and >= 0");
        return WLSQM_EVALUE;
    }
    if (maxiter < 0 || maxiter > INT32_MAX) { set_error("krylov_l2_start: maxiter must be 0 .. 2^31 - 1"); return WLSQM_EVALUE; }
    DeviceScope scope;
    rc = scope.enter(device);
    if (rc != WLSQM_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const KrylovL2Work w = krylov_l2_work(workspace, nrows, precond);
    const dim3 grid((unsigned)w.nwg);
    if (precond == 1) {
        hipLaunchKernelGGL(krylov_diag_kernel, grid, dim3(256), 0, s, m, w.dinv, w.partial);
        note_kernel("krylov-diag");
    }
    const double* counts = precond > 1 ? static_cast<const double*>(planes) + krylov_plane_doubles(nslices, precond) : w.partial;
    hipLaunchKernelGGL(krylov_reduce_kernel, dim3(1), dim3(256), 0, s, (int)REDUCE_DIAG, counts, precond ? w.nwg : 0LL, 1, w.sc, rtol, atol,
                       (int)maxiter);
    hipLaunchKernelGGL((krylov_spmv_kernel<SPMV_RESIDUAL>), grid, dim3(256), 0, s, m, x, b, w.r, w.rt, w.partial, (const KrylovScalars*)w.sc, 0);
    note_kernel("krylov-spmv-dot");
    hipLaunchKernelGGL(krylov_l2_reduce_kernel, dim3(1), dim3(256), 0, s, (int)L2_START, (const double*)w.partial, w.nwg, w.sc, rtol, atol);
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("krylov-l2-reduce");
    return WLSQM_OK;
}

int wlsqm_hip_krylov_l2_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                               const int32_t* col, const double* val, const double* diag, double diag_const, double scale, int precond,
                               const void* planes, double* x, int64_t ncycles, void* workspace, int device, void* stream) {
    KrylovSys m;
    int rc = krylov_system("krylov_l2", m, nrows, nslices, len, width, soff, col, val, diag, diag_const, scale, workspace);
    if (rc != WLSQM_OK) return rc;
    rc = krylov_many_arguments("krylov_l2", nrows, nslices, 1, precond, planes, workspace);
    if (rc != WLSQM_OK) return rc;
    if (!x) { set_error("krylov_l2: null array"); return WLSQM_EVALUE; }
    if (ncycles < 0) { set_error("krylov_l2: ncycles must be >= 0"); return WLSQM_EVALUE; }
    DeviceScope scope;
    rc = scope.enter(device);
    if (rc != WLSQM_OK || ncycles == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    const KrylovL2Work w = krylov_l2_work(workspace, nrows, precond);
    const double* W = static_cast<const double*>(planes);
    switch (precond) {
    case 8: krylov_l2_cycles<8>(m, w, W, x, ncycles, s); break;
    case 16: krylov_l2_cycles<16>(m, w, W, x, ncycles, s); break;
    case 32: krylov_l2_cycles<32>(m, w, W, x, ncycles, s); break;
    default: krylov_l2_cycles<0>(m, w, nullptr, x, ncycles, s); break;
    }
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel(precond > 1 ? "krylov-l2-update-block" : "krylov-l2-update");
    return WLSQM_OK;
}

int64_t wlsqm_hip_krylov_spai_bytes(int64_t nrows, int64_t total) {
    if (nrows < 0 || total < 0) return -1;
    return (int64_t)sizeof(double) * (nrows + (nrows + 63) / 64 + total);
}

int wlsqm_hip_krylov_spai_build_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                       const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                       int max_width, void* planes, int64_t npairs, const int32_t* pair_dest, const int32_t* pair_src,
                                       void* planes_t, int device, void* stream) {
    KrylovSys m;
    int rc = krylov_spai_arguments("krylov_spai_build", nrows, nslices, planes);
    if (rc != WLSQM_OK) return rc;
    rc = krylov_system("krylov_spai_build", m, nrows, nslices, len, width, soff, col, val, diag, diag_const, scale, planes);
    if (rc != WLSQM_OK) return rc;
    if (max_width < 0 || max_width > KRYLOV_SPAI_CAP) {
        set_error("krylov_spai_build: max_width must be 0 .. 65, the widest slice of the matrix");
        return WLSQM_EVALUE;
    }
    if (planes_t && (npairs < 0 || (npairs > 0 && (!pair_dest || !pair_src)))) { set_error("krylov_spai_build: null array"); return WLSQM_EVALUE; }
    DeviceScope scope;
    rc = scope.enter(device);
    if (rc != WLSQM_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const KrylovSpai p = krylov_spai_planes(planes, nrows);
    const dim3 grid((unsigned)nslices);
    if (max_width <= 16) hipLaunchKernelGGL(krylov_spai_kernel<16>, grid, dim3(64), 0, s, m, p.qd, p.qv, p.counts);
    else if (max_width <= 28) hipLaunchKernelGGL(krylov_spai_kernel<28>, grid, dim3(64), 0, s, m, p.qd, p.qv, p.counts);
    else if (max_width <= 44) hipLaunchKernelGGL(krylov_spai_kernel<44>, grid, dim3(64), 0, s, m, p.qd, p.qv, p.counts);
    else hipLaunchKernelGGL(krylov_spai_kernel<64>, grid, dim3(64), 0, s, m, p.qd, p.qv, p.counts);
    if (planes_t) {
        const long long head = nrows + nslices, most = head > npairs ? head : npairs;
        hipLaunchKernelGGL(krylov_spai_transpose_kernel, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, s, (long long)npairs, pair_dest,
                           pair_src, head, (const double*)planes, static_cast<double*>(planes_t));
    }
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("krylov-spai");
    return WLSQM_OK;
}

int wlsqm_hip_krylov_spai_apply_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                       const int32_t* col, const void* planes, const double* v, double* out, int device, void* stream) {
    KrylovSys m;
    int rc = krylov_spai_arguments("krylov_spai_apply", nrows, nslices, planes);
    if (rc != WLSQM_OK) return rc;
    const KrylovSpai p = krylov_spai_planes(planes, nrows < 0 ? 0 : nrows);
    rc = krylov_system("krylov_spai_apply", m, nrows, nslices, len, width, soff, col, p.qv, p.qd, 0.0, 1.0, planes);
    if (rc != WLSQM_OK) return rc;
    if (!v || !out) { set_error("krylov_spai_apply: null array"); return WLSQM_EVALUE; }
    DeviceScope scope;
    rc = scope.enter(device);
    if (rc != WLSQM_OK) return rc;
    krylov_spai_apply(m, (nrows + 255) / 256, v, out, nullptr, nullptr, 1, (hipStream_t)stream);
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("krylov-spai-apply");
    return WLSQM_OK;
}

int wlsqm_hip_krylov_spai_start_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                       const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                       int l2, const void* planes, const double* b, const double* x, double rtol, double atol,
                                       int64_t maxiter, void* workspace, int device, void* stream) {
    KrylovSys m;
    int rc = krylov_spai_arguments("krylov_spai_start", nrows, nslices, planes);
    if (rc != WLSQM_OK) return rc;
    rc = krylov_system("krylov_spai_start", m, nrows, nslices, len, width, soff, col, val, diag, diag_const, scale, workspace);
    if (rc != WLSQM_OK) return rc;
    rc = krylov_tolerances("krylov_spai_start", b, x, rtol, atol, maxiter);
    if (rc != WLSQM_OK) return rc;
    DeviceScope scope;
    rc = scope.enter(device);
    if (rc != WLSQM_OK) return rc;
    const KrylovSpai p = krylov_spai_planes(planes, nrows);
    return krylov_applied_start(m, p.counts, nslices, l2, b, x, rtol, atol, maxiter, workspace, (hipStream_t)stream);
}

int wlsqm_hip_krylov_spai_iterate_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                         const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                         int l2, const void* planes, double* x, int64_t niter, void* workspace, int device, void* stream) {
    KrylovSys m;
    int rc = krylov_spai_arguments("krylov_spai_iterate", nrows, nslices, planes);
    if (rc != WLSQM_OK) return rc;
    rc = krylov_system("krylov_spai_iterate", m, nrows, nslices, len, width, soff, col, val, diag, diag_const, scale, workspace);
    if (rc != WLSQM_OK) return rc;
    if (!x) { set_error("krylov_spai_iterate: null array"); return WLSQM_EVALUE; }
    if (niter < 0) { set_error("krylov_spai_iterate: niter must be >= 0"); return WLSQM_EVALUE; }
    DeviceScope scope;
    rc = scope.enter(device);
    if (rc != WLSQM_OK || niter == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    const KrylovSys q = krylov_spai_system(m, krylov_spai_planes(planes, nrows));
    const long long nwg = (nrows + 255) / 256;
    const KrylovScalars* sc = static_cast<const KrylovScalars*>(workspace);
    krylov_applied_run(m, [&](const double* in, double* out, double* acc) { krylov_spai_apply(q, nwg, in, out, acc, sc, 0, s); }, l2, x,
                       niter, workspace, s);
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel(l2 ? "krylov-spai-l2-update" : "krylov-spai-update");
    return WLSQM_OK;
}

int64_t wlsqm_hip_krylov_schwarz_bytes(int64_t nrows, int block, int rows) {
    if (nrows < 0 || (block != 8 && block != 16 && block != 32) || (rows != 32 && rows != 64) || rows <= block) return -1;
    const int64_t nslices = (nrows + 63) / 64;
    return (int64_t)sizeof(double) * (nslices * rows * 64 + nslices * (64 / block));
}

int wlsqm_hip_krylov_schwarz_build_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                          const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                          int block, int rows, const int32_t* table, void* planes, void* planes_t, int device,
                                          void* stream) {
    KrylovSys m;
    int rc = krylov_schwarz_arguments("krylov_schwarz_build", nrows, nslices, block, rows, table, planes);
    if (rc != WLSQM_OK) return rc;
    rc = krylov_system("krylov_schwarz_build", m, nrows, nslices, len, width, soff, col, val, diag, diag_const, scale, planes);
    if (rc != WLSQM_OK) return rc;
    DeviceScope scope;
    rc = scope.enter(device);
    if (rc != WLSQM_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const KrylovSchwarz p = krylov_schwarz_planes(planes, nrows, nslices, block, rows);
    const KrylovSchwarz t = krylov_schwarz_planes(planes_t, nrows, nslices, block, rows);
    const dim3 grid((unsigned)p.nslots);
    if (rows == 32) hipLaunchKernelGGL(krylov_schwarz_build_kernel<32>, grid, dim3(64), 0, s, m, p, table, t.W, t.counts);
    else hipLaunchKernelGGL(krylov_schwarz_build_kernel<64>, grid, dim3(64), 0, s, m, p, table, t.W, t.counts);
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("krylov-schwarz-build");
    return WLSQM_OK;
}

int wlsqm_hip_krylov_schwarz_apply_device(int64_t nrows, int block, int rows, const int32_t* table, const void* planes, const double* v,
                                          double* out, int device, void* stream) {
    int rc = krylov_schwarz_arguments("krylov_schwarz_apply", nrows, (nrows + 63) / 64, block, rows, table, planes);
    if (rc != WLSQM_OK) return rc;
    if (!v || !out) { set_error("krylov_schwarz_apply: null array"); return WLSQM_EVALUE; }
    DeviceScope scope;
    rc = scope.enter(device);
    if (rc != WLSQM_OK) return rc;
    krylov_schwarz_apply(krylov_schwarz_planes(planes, nrows, (nrows + 63) / 64, block, rows), table, nrows, v, out, nullptr, nullptr, 1,
                         (hipStream_t)stream);
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("krylov-schwarz-apply");
    return WLSQM_OK;
}

int wlsqm_hip_krylov_schwarz_start_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                          const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                          int l2, int block, int rows, const int32_t* table, const void* planes, const double* b,
                                          const double* x, double rtol, double atol, int64_t maxiter, void* workspace, int device,
                                          void* stream) {
    KrylovSys m;
    int rc = krylov_schwarz_arguments("krylov_schwarz_start", nrows, nslices, block, rows, table, planes);
    if (rc != WLSQM_OK) return rc;
    rc = krylov_system("krylov_schwarz_start", m, nrows, nslices, len, width, soff, col, val, diag, diag_const, scale, workspace);
    if (rc != WLSQM_OK) return rc;
    rc = krylov_tolerances("krylov_schwarz_start", b, x, rtol, atol, maxiter);
    if (rc != WLSQM_OK) return rc;
    DeviceScope scope;
    rc = scope.enter(device);
    if (rc != WLSQM_OK) return rc;
    const KrylovSchwarz p = krylov_schwarz_planes(planes, nrows, nslices, block, rows);
    return krylov_applied_start(m, p.counts, p.nslots, l2, b, x, rtol, atol, maxiter, workspace, (hipStream_t)stream);
}

int wlsqm_hip_krylov_schwarz_iterate_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                            const int32_t* col, const double* val, const double* diag, double diag_const, double scale,
                                            int l2, int block, int rows, const int32_t* table, const void* planes, double* x,
                                            int64_t niter, void* workspace, int device, void* stream) {
    KrylovSys m;
    int rc = krylov_schwarz_arguments("krylov_schwarz_iterate", nrows, nslices, block, rows, table, planes);
    if (rc != WLSQM_OK) return rc;
    rc = krylov_system("krylov_schwarz_iterate", m, nrows, nslices, len, width, soff, col, val, diag, diag_const, scale, workspace);
    if (rc != WLSQM_OK) return rc;
    if (!x) { set_error("krylov_schwarz_iterate: null array"); return WLSQM_EVALUE; }
    if (niter < 0) { set_error("krylov_schwarz_iterate: niter must be >= 0"); return WLSQM_EVALUE; }
    DeviceScope scope;
    rc = scope.enter(device);
    if (rc != WLSQM_OK || niter == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    const KrylovSchwarz p = krylov_schwarz_planes(planes, nrows, nslices, block, rows);
    const KrylovScalars* sc = static_cast<const KrylovScalars*>(workspace);
    krylov_applied_run(m, [&](const double* in, double* out, double* acc) { krylov_schwarz_apply(p, table, nrows, in, out, acc, sc, 0, s); },
                       l2, x, niter, workspace, s);
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel(l2 ? "krylov-schwarz-l2-update" : "krylov-schwarz-update");
    return WLSQM_OK;
}

int64_t wlsqm_hip_krylov_system_workspace_bytes(int64_t npoints, int m) {
    if (npoints < 0 || m < 1 || m > KRYLOV_SYSTEM_FIELDS) return -1;
    return wlsqm_hip_krylov_workspace_bytes(npoints * m);
}

int wlsqm_hip_krylov_system_start_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                         const int32_t* col, const double* val, int64_t total, int nop, int m, const double* coupling,
                                         const double* diag, const double* diag_const, int jacobi, const double* b, const double* x,
                                         double rtol, double atol, int64_t maxiter, void* workspace, int device, void* stream) {
    int rc = krylov_tolerances("krylov_system_start", b, x, rtol, atol, maxiter);
    if (rc != WLSQM_OK) return rc;
    KrylovSystemCall c;
    c.what = SYSTEM_CALL_START; c.jacobi = jacobi; c.maxiter = (int)maxiter;
    c.in = x; c.other = b; c.x = const_cast<double*>(x);        // the start reads x
    c.rtol = rtol; c.atol = atol; c.niter = 0; c.s = (hipStream_t)stream;
    return krylov_system_call("krylov_system_start", c, npoints, nslices, len, width, soff, col, val, total, nop, m, coupling, diag,
                              diag_const, workspace, device);
}

int wlsqm_hip_krylov_system_bicgstab_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                            const int32_t* col, const double* val, int64_t total, int nop, int m, const double* coupling,
                                            const double* diag, const double* diag_const, int jacobi, double* x, int64_t niter,
                                            void* workspace, int device, void* stream) {
    if (niter < 0) { set_error("krylov_system_bicgstab: niter must be >= 0"); return WLSQM_EVALUE; }
    KrylovSystemCall c;
    c.what = SYSTEM_CALL_ITERATE; c.jacobi = jacobi; c.maxiter = 0;
    c.in = x; c.other = x; c.x = x;
    c.rtol = c.atol = 0.0; c.niter = niter; c.s = (hipStream_t)stream;
    return krylov_system_call("krylov_system_bicgstab", c, npoints, nslices, len, width, soff, col, val, total, nop, m, coupling, diag,
                              diag_const, workspace, device);
}

int wlsqm_hip_krylov_system_product_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                           const int32_t* col, const double* val, int64_t total, int nop, int m, const double* coupling,
                                           const double* diag, const double* diag_const, const double* in, const double* w, double* out,
                                           void* workspace, int device, void* stream) {
    KrylovSystemCall c;
    c.what = SYSTEM_CALL_PRODUCT; c.jacobi = 0; c.maxiter = 0;
    c.in = in; c.other = w; c.x = out;
    c.rtol = c.atol = 0.0; c.niter = 0; c.s = (hipStream_t)stream;
    return krylov_system_call("krylov_system_product", c, npoints, nslices, len, width, soff, col, val, total, nop, m, coupling, diag,
                              diag_const, workspace, device);
}

// M^T: the three calls above on the transposed arrays of the planes; coupling, diag and diag_const are the forward system's own.
int wlsqm_hip_krylov_system_start_transposed_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                                    const int64_t* soff, const int32_t* col, const double* val, int64_t total, int nop, int m,
                                                    const double* coupling, const double* diag, const double* diag_const, int jacobi,
                                                    const double* b, const double* x, double rtol, double atol, int64_t maxiter,
                                                    void* workspace, int device, void* stream) {
    int rc = krylov_tolerances("krylov_system_start_transposed", b, x, rtol, atol, maxiter);
    if (rc != WLSQM_OK) return rc;
    KrylovSystemCall c;
    c.what = SYSTEM_CALL_START; c.jacobi = jacobi; c.maxiter = (int)maxiter;
    c.in = x; c.other = b; c.x = const_cast<double*>(x);
    c.rtol = rtol; c.atol = atol; c.niter = 0; c.s = (hipStream_t)stream;
    return krylov_system_call("krylov_system_start_transposed", c, npoints, nslices, len, width, soff, col, val, total, nop, m, coupling,
                              diag, diag_const, workspace, device, true);
}

int wlsqm_hip_krylov_system_bicgstab_transposed_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                                       const int64_t* soff, const int32_t* col, const double* val, int64_t total, int nop,
                                                       int m, const double* coupling, const double* diag, const double* diag_const,
                                                       int jacobi, double* x, int64_t niter, void* workspace, int device, void* stream) {
    if (niter < 0) { set_error("krylov_system_bicgstab_transposed: niter must be >= 0"); return WLSQM_EVALUE; }
    KrylovSystemCall c;
    c.what = SYSTEM_CALL_ITERATE; c.jacobi = jacobi; c.maxiter = 0;
    c.in = x; c.other = x; c.x = x;
    c.rtol = c.atol = 0.0; c.niter = niter; c.s = (hipStream_t)stream;
    return krylov_system_call("krylov_system_bicgstab_transposed", c, npoints, nslices, len, width, soff, col, val, total, nop, m, coupling,
                              diag, diag_const, workspace, device, true);
}

int wlsqm_hip_krylov_system_product_transposed_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                                      const int64_t* soff, const int32_t* col, const double* val, int64_t total, int nop,
                                                      int m, const double* coupling, const double* diag, const double* diag_const,
                                                      const double* in, const double* w, double* out, void* workspace, int device,
                                                      void* stream) {
    KrylovSystemCall c;
    c.what = SYSTEM_CALL_PRODUCT; c.jacobi = 0; c.maxiter = 0;
    c.in = in; c.other = w; c.x = out;
    c.rtol = c.atol = 0.0; c.niter = 0; c.s = (hipStream_t)stream;
    return krylov_system_call("krylov_system_product_transposed", c, npoints, nslices, len, width, soff, col, val, total, nop, m, coupling,
                              diag, diag_const, workspace, device, true);
}

int wlsqm_hip_krylov_system_grads_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                         const int32_t* col, int64_t total, int nop, int m, const double* coupling, const double* lam,
                                         const double* x, double* grad_val, double* grad_diag, int device, void* stream) {
    return krylov_system_grads_call("krylov_system_grads", false, npoints, nslices, len, width, soff, col, total, nop, m, coupling, lam, x,
                                    grad_val, grad_diag, device, stream);
}

// A per-point coupling: `coupling` is a device tensor (m, m, nop, npoints).  transposed != 0: the arrays are the
// transposed ones of the planes and `mixed` is a device plane of nop * m * npoints doubles that every product writes first.
int wlsqm_hip_krylov_system_point_start_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                               const int32_t* col, const double* val, int64_t total, int nop, int m, const double* coupling,
                                               const double* diag, const double* diag_const, int transposed, double* mixed, int jacobi,
                                               const double* b, const double* x, double rtol, double atol, int64_t maxiter, void* workspace,
                                               int device, void* stream) {
    int rc = krylov_tolerances("krylov_system_point_start", b, x, rtol, atol, maxiter);
    if (rc != WLSQM_OK) return rc;
    KrylovPointCall p;
    KrylovSystemCall& c = p.c;
    p.mixed = mixed;
    c.what = SYSTEM_CALL_START; c.jacobi = jacobi; c.maxiter = (int)maxiter;
    c.in = x; c.other = b; c.x = const_cast<double*>(x);        // the start reads x
    c.rtol = rtol; c.atol = atol; c.niter = 0; c.s = (hipStream_t)stream;
    return krylov_point_call("krylov_system_point_start", p, npoints, nslices, len, width, soff, col, val, total, nop, m, coupling, diag,
                             diag_const, transposed, workspace, device);
}

int wlsqm_hip_krylov_system_point_bicgstab_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                                  const int64_t* soff, const int32_t* col, const double* val, int64_t total, int nop, int m,
                                                  const double* coupling, const double* diag, const double* diag_const, int transposed,
                                                  double* mixed, int jacobi, double* x, int64_t niter, void* workspace, int device,
                                                  void* stream) {
    if (niter < 0) { set_error("krylov_system_point_bicgstab: niter must be >= 0"); return WLSQM_EVALUE; }
    KrylovPointCall p;
    KrylovSystemCall& c = p.c;
    p.mixed = mixed;
    c.what = SYSTEM_CALL_ITERATE; c.jacobi = jacobi; c.maxiter = 0;
    c.in = x; c.other = x; c.x = x;
    c.rtol = c.atol = 0.0; c.niter = niter; c.s = (hipStream_t)stream;
    return krylov_point_call("krylov_system_point_bicgstab", p, npoints, nslices, len, width, soff, col, val, total, nop, m, coupling, diag,
                             diag_const, transposed, workspace, device);
}

int wlsqm_hip_krylov_system_point_product_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                                 const int64_t* soff, const int32_t* col, const double* val, int64_t total, int nop, int m,
                                                 const double* coupling, const double* diag, const double* diag_const, int transposed,
                                                 double* mixed, const double* in, const double* w, double* out, void* workspace, int device,
                                                 void* stream) {
    KrylovPointCall p;
    KrylovSystemCall& c = p.c;
    p.mixed = mixed;
    c.what = SYSTEM_CALL_PRODUCT; c.jacobi = 0; c.maxiter = 0;
    c.in = in; c.other = w; c.x = out;
    c.rtol = c.atol = 0.0; c.niter = 0; c.s = (hipStream_t)stream;
    return krylov_point_call("krylov_system_point_product", p, npoints, nslices, len, width, soff, col, val, total, nop, m, coupling, diag,
                             diag_const, transposed, workspace, device);
}

int wlsqm_hip_krylov_system_point_grads_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                               const int32_t* col, int64_t total, int nop, int m, const double* coupling, const double* lam,
                                               const double* x, double* grad_val, double* grad_diag, int device, void* stream) {
    return krylov_system_grads_call("krylov_system_point_grads", true, npoints, nslices, len, width, soff, col, total, nop, m, coupling, lam, x,
                                    grad_val, grad_diag, device, stream);
}

// Blocks over points.  `points` points of m unknowns each make a block, m points <= 32.
int64_t wlsqm_hip_krylov_system_block_bytes(int64_t npoints, int m, int points) {
    if (npoints < 0 || m < 1 || m > KRYLOV_SYSTEM_FIELDS || points < 1 || m * points > 32) return -1;
    const long long nwaves = npoints ? krylov_system_block_waves(npoints, m, points) : 0;
    return (int64_t)sizeof(double) * (nwaves * krylov_system_block_nb(m * points) * 64 + (nwaves + 3) / 4);
}

// "krylov-system-blocks", one launch: the forward arrays, the host table (point == 0) or the device tensor (point != 0), diag; the
// inverses into `planes` and, when given, their transposes into `planes_t`.
static int krylov_system_block_build(const char* who, int invert, int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                     const int64_t* soff, const int32_t* col, const double* val, int64_t total, int nop, int m,
                                     const double* coupling, const double* diag, const double* diag_const, int point, int points,
                                     void* planes, void* planes_t, int device, void* stream) {
    const std::string name(who);
    int rc = krylov_system_block_arguments(who, m, points, planes, planes_t);
    if (rc != WLSQM_OK) return rc;
    if (nop < 1 || nop > KRYLOV_SYSTEM_PLANES) { set_error(name + ": nop must be 1 .. 8"); return WLSQM_EVALUE; }
    if (npoints < 1 || nslices < 0 || npoints > 64 * nslices || total < 0 || (npoints * m + 255) / 256 > 0x7fffffffLL) {
        set_error(name + ": npoints must be 1 .. 64 * nslices");
        return WLSQM_EVALUE;
    }
    if (!len || !width || !soff || !col || !val || !coupling || (!diag && !diag_const)) { set_error(name + ": null array"); return WLSQM_EVALUE; }
    if (point && ((uintptr_t)coupling & 7)) { set_error(name + ": coupling must be 8-byte aligned"); return WLSQM_EVALUE; }
    KrylovCoupled q;
    q.npoints = npoints; q.total = total;
    q.len = len; q.width = width; q.soff = reinterpret_cast<const long long*>(soff);
    q.col = col; q.val = val; q.dten = diag; q.dswap = 0; q.cpt = point ? coupling : nullptr;
    for (int i = 0; i < KRYLOV_SYSTEM_FIELDS * KRYLOV_SYSTEM_FIELDS; ++i) q.dconst[i] = (!diag && i < m * m) ? diag_const[i] : 0.0;
    for (int i = 0; i < KRYLOV_SYSTEM_FIELDS * KRYLOV_SYSTEM_FIELDS * KRYLOV_SYSTEM_PLANES; ++i) q.coupling[i] = (!point && i < m * m * nop) ? coupling[i] : 0.0;
    DeviceScope scope;
    rc = scope.enter(device);
    if (rc != WLSQM_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const long long nwaves = krylov_system_block_waves(npoints, m, points);
    const dim3 grid((unsigned)((nwaves + 3) / 4));
    double *W = static_cast<double*>(planes), *WT = static_cast<double*>(planes_t);
    switch (krylov_system_block_nb(m * points)) {
    case 8: hipLaunchKernelGGL(krylov_system_blocks_kernel<8>, grid, dim3(256), 0, s, q, m, nop, points, nwaves, invert, W, WT); break;
    case 16: hipLaunchKernelGGL(krylov_system_blocks_kernel<16>, grid, dim3(256), 0, s, q, m, nop, points, nwaves, invert, W, WT); break;
    default: hipLaunchKernelGGL(krylov_system_blocks_kernel<32>, grid, dim3(256), 0, s, q, m, nop, points, nwaves, invert, W, WT); break;
    }
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("krylov-system-blocks");
    return WLSQM_OK;
}

int wlsqm_hip_krylov_system_block_factor_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                                const int64_t* soff, const int32_t* col, const double* val, int64_t total, int nop, int m,
                                                const double* coupling, const double* diag, const double* diag_const, int point, int points,
                                                void* planes, void* planes_t, int device, void* stream) {
    return krylov_system_block_build("krylov_system_block_factor", 1, npoints, nslices, len, width, soff, col, val, total, nop, m, coupling,
                                     diag, diag_const, point, points, planes, planes_t, device, stream);
}

// The same launch without the elimination: the gathered diagonal blocks of M themselves in the plane's layout, for checks.
int wlsqm_hip_krylov_system_block_gather_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                                const int64_t* soff, const int32_t* col, const double* val, int64_t total, int nop, int m,
                                                const double* coupling, const double* diag, const double* diag_const, int point, int points,
                                                void* planes, int device, void* stream) {
    return krylov_system_block_build("krylov_system_block_gather", 0, npoints, nslices, len, width, soff, col, val, total, nop, m, coupling,
                                     diag, diag_const, point, points, planes, nullptr, device, stream);
}

// "krylov-system-precondition", one launch: out = P v on (npoints, m) vectors; the plane of the transposes gives P^T v.
int wlsqm_hip_krylov_system_block_precondition_device(int64_t npoints, int m, int points, const void* planes, const double* v, double* out,
                                                      int device, void* stream) {
    int rc = krylov_system_block_arguments("krylov_system_block_precondition", m, points, planes, nullptr);
    if (rc != WLSQM_OK) return rc;
    if (npoints < 1 || (npoints * m + 255) / 256 > 0x7fffffffLL) {
        set_error("krylov_system_block_precondition: npoints must be >= 1");
        return WLSQM_EVALUE;
    }
    if (!v || !out) { set_error("krylov_system_block_precondition: null array"); return WLSQM_EVALUE; }
    DeviceScope scope;
    rc = scope.enter(device);
    if (rc != WLSQM_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int rows = m * points;
    const long long nrows = npoints * m, nwaves = krylov_system_block_waves(npoints, m, points);
    const dim3 grid((unsigned)((nwaves + 3) / 4));
    const double* W = static_cast<const double*>(planes);
    switch (krylov_system_block_nb(rows)) {
    case 8: hipLaunchKernelGGL(krylov_system_precondition_kernel<8>, grid, dim3(256), 0, s, nrows, rows, nwaves, W, v, out); break;
    case 16: hipLaunchKernelGGL(krylov_system_precondition_kernel<16>, grid, dim3(256), 0, s, nrows, rows, nwaves, W, v, out); break;
    default: hipLaunchKernelGGL(krylov_system_precondition_kernel<32>, grid, dim3(256), 0, s, nrows, rows, nwaves, W, v, out); break;
    }
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("krylov-system-precondition");
    return WLSQM_OK;
}

// wlsqm_hip_krylov_system_start_device / _bicgstab_device and their transposed forms with P taken from `planes` (the transposed forms:
// from the plane of the transposes) as the factor left it.
int wlsqm_hip_krylov_system_block_start_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                               const int32_t* col, const double* val, int64_t total, int nop, int m, const double* coupling,
                                               const double* diag, const double* diag_const, int points, const void* planes, const double* b,
                                               const double* x, double rtol, double atol, int64_t maxiter, void* workspace, int device,
                                               void* stream) {
    int rc = krylov_system_block_arguments("krylov_system_block_start", m, points, planes, nullptr);
    if (rc != WLSQM_OK) return rc;
    rc = krylov_tolerances("krylov_system_block_start", b, x, rtol, atol, maxiter);
    if (rc != WLSQM_OK) return rc;
    KrylovSystemCall c;
    c.points = points; c.W = static_cast<const double*>(planes);
    c.what = SYSTEM_CALL_START; c.jacobi = 1; c.maxiter = (int)maxiter;
    c.in = x; c.other = b; c.x = const_cast<double*>(x);
    c.rtol = rtol; c.atol = atol; c.niter = 0; c.s = (hipStream_t)stream;
    return krylov_system_call("krylov_system_block_start", c, npoints, nslices, len, width, soff, col, val, total, nop, m, coupling, diag,
                              diag_const, workspace, device);
}

int wlsqm_hip_krylov_system_block_bicgstab_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                                  const int64_t* soff, const int32_t* col, const double* val, int64_t total, int nop, int m,
                                                  const double* coupling, const double* diag, const double* diag_const, int points,
                                                  const void* planes, double* x, int64_t niter, void* workspace, int device, void* stream) {
    int rc = krylov_system_block_arguments("krylov_system_block_bicgstab", m, points, planes, nullptr);
    if (rc != WLSQM_OK) return rc;
    if (niter < 0) { set_error("krylov_system_block_bicgstab: niter must be >= 0"); return WLSQM_EVALUE; }
    KrylovSystemCall c;
    c.points = points; c.W = static_cast<const double*>(planes);
    c.what = SYSTEM_CALL_ITERATE; c.jacobi = 1; c.maxiter = 0;
    c.in = x; c.other = x; c.x = x;
    c.rtol = c.atol = 0.0; c.niter = niter; c.s = (hipStream_t)stream;
    return krylov_system_call("krylov_system_block_bicgstab", c, npoints, nslices, len, width, soff, col, val, total, nop, m, coupling, diag,
                              diag_const, workspace, device);
}

int wlsqm_hip_krylov_system_block_start_transposed_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                                          const int64_t* soff, const int32_t* col, const double* val, int64_t total, int nop,
                                                          int m, const double* coupling, const double* diag, const double* diag_const,
                                                          int points, const void* planes, const double* b, const double* x, double rtol,
                                                          double atol, int64_t maxiter, void* workspace, int device, void* stream) {
    int rc = krylov_system_block_arguments("krylov_system_block_start_transposed", m, points, planes, nullptr);
    if (rc != WLSQM_OK) return rc;
    rc = krylov_tolerances("krylov_system_block_start_transposed", b, x, rtol, atol, maxiter);
    if (rc != WLSQM_OK) return rc;
    KrylovSystemCall c;
    c.points = points; c.W = static_cast<const double*>(planes);
    c.what = SYSTEM_CALL_START; c.jacobi = 1; c.maxiter = (int)maxiter;
    c.in = x; c.other = b; c.x = const_cast<double*>(x);
    c.rtol = rtol; c.atol = atol; c.niter = 0; c.s = (hipStream_t)stream;
    return krylov_system_call("krylov_system_block_start_transposed", c, npoints, nslices, len, width, soff, col, val, total, nop, m,
                              coupling, diag, diag_const, workspace, device, true);
}

int wlsqm_hip_krylov_system_block_bicgstab_transposed_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                                             const int64_t* soff, const int32_t* col, const double* val, int64_t total,
                                                             int nop, int m, const double* coupling, const double* diag,
                                                             const double* diag_const, int points, const void* planes, double* x,
                                                             int64_t niter, void* workspace, int device, void* stream) {
    int rc = krylov_system_block_arguments("krylov_system_block_bicgstab_transposed", m, points, planes, nullptr);
    if (rc != WLSQM_OK) return rc;
    if (niter < 0) { set_error("krylov_system_block_bicgstab_transposed: niter must be >= 0"); return WLSQM_EVALUE; }
    KrylovSystemCall c;
    c.points = points; c.W = static_cast<const double*>(planes);
    c.what = SYSTEM_CALL_ITERATE; c.jacobi = 1; c.maxiter = 0;
    c.in = x; c.other = x; c.x = x;
    c.rtol = c.atol = 0.0; c.niter = niter; c.s = (hipStream_t)stream;
    return krylov_system_call("krylov_system_block_bicgstab_transposed", c, npoints, nslices, len, width, soff, col, val, total, nop, m,
                              coupling, diag, diag_const, workspace, device, true);
}

// The same for a per-point coupling: wlsqm_hip_krylov_system_point_start_device / _bicgstab_device with the blocks.
int wlsqm_hip_krylov_system_point_block_start_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                                     const int64_t* soff, const int32_t* col, const double* val, int64_t total, int nop, int m,
                                                     const double* coupling, const double* diag, const double* diag_const, int transposed,
                                                     double* mixed, int points, const void* planes, const double* b, const double* x,
                                                     double rtol, double atol, int64_t maxiter, void* workspace, int device, void* stream) {
    int rc = krylov_system_block_arguments("krylov_system_point_block_start", m, points, planes, nullptr);
    if (rc != WLSQM_OK) return rc;
    rc = krylov_tolerances("krylov_system_point_block_start", b, x, rtol, atol, maxiter);
    if (rc != WLSQM_OK) return rc;
    KrylovPointCall p;
    KrylovSystemCall& c = p.c;
    p.mixed = mixed;
    c.points = points; c.W = static_cast<const double*>(planes);
    c.what = SYSTEM_CALL_START; c.jacobi = 1; c.maxiter = (int)maxiter;
    c.in = x; c.other = b; c.x = const_cast<double*>(x);
    c.rtol = rtol; c.atol = atol; c.niter = 0; c.s = (hipStream_t)stream;
    return krylov_point_call("krylov_system_point_block_start", p, npoints, nslices, len, width, soff, col, val, total, nop, m, coupling,
                             diag, diag_const, transposed, workspace, device);
}

int wlsqm_hip_krylov_system_point_block_bicgstab_device(int64_t npoints, int64_t nslices, const int32_t* len, const int32_t* width,
                                                        const int64_t* soff, const int32_t* col, const double* val, int64_t total, int nop,
                                                        int m, const double* coupling, const double* diag, const double* diag_const,
                                                        int transposed, double* mixed, int points, const void* planes, double* x,
                                                        int64_t niter, void* workspace, int device, void* stream) {
    int rc = krylov_system_block_arguments("krylov_system_point_block_bicgstab", m, points, planes, nullptr);
    if (rc != WLSQM_OK) return rc;
    if (niter < 0) { set_error("krylov_system_point_block_bicgstab: niter must be >= 0"); return WLSQM_EVALUE; }
    KrylovPointCall p;
    KrylovSystemCall& c = p.c;
    p.mixed = mixed;
    c.points = points; c.W = static_cast<const double*>(planes);
    c.what = SYSTEM_CALL_ITERATE; c.jacobi = 1; c.maxiter = 0;
    c.in = x; c.other = x; c.x = x;
    c.rtol = c.atol = 0.0; c.niter = niter; c.s = (hipStream_t)stream;
    return krylov_point_call("krylov_system_point_block_bicgstab", p, npoints, nslices, len, width, soff, col, val, total, nop, m, coupling,
                             diag, diag_const, transposed, workspace, device);
}

}  // extern "C"
