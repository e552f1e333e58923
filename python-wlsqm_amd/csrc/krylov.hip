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
    const double s0 = sums[0], s1 = sums[1];
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

}  // extern "C"
