// lapack_batched.hip — batched small dense solves of wlsqm.utils.lapackdrivers: LU with partial pivoting (dgetf2 / dgetrs
// semantics) and Bunch-Kaufman U*D*U^T (dsytf2 / dsytrs, uplo = 'U'), over `count` independent problems in the reference's
// Fortran layout: A (n, n, nlhs), b (n, count), ipiv (n, nlhs) 1-based, info one per factored matrix.
//
// Two forms, chosen by n alone (never by count or stream), so a matrix gives the same bits wherever it sits in a batch:
//   LANE  (n <= LANE_NMAX): one lane per problem, a wave per 64 problems.  The wave's 64 matrices (a contiguous run of
//         64*n*n doubles) are staged through LDS with wave-wide contiguous loads and stores, transposed so that element e of
//         lane q sits at e*LP + q: every step of the sequential factorization is one conflict-free LDS access per lane, and
//         the data-dependent pivot rows are plain LDS addresses (nothing is indexed in registers, so nothing goes to scratch).
//   GROUP (n > LANE_NMAX): one workgroup per problem.  The matrix lives in LDS while it fits in 64 KiB (n <= GROUP_LDS_NMAX),
//         and is factored in place in global memory above that.  Threads split every column / rank-1 / rank-2 update; the
//         pivot searches are block reductions in which the first largest entry wins (idamax).
// The solves take one right-hand side per problem; with lhs_stride 0 every right-hand side uses the one factor (generals).
#include <cfloat>
#include <climits>
#include <cstring>

#include "wlsqm_dispatch.hpp"
#include "hostio.hpp"

namespace wlsqm {
namespace lapack {

constexpr int LANE_NMAX = 8;        // lane form up to here
constexpr int GROUP_LDS_NMAX = 89;  // group form keeps A in LDS up to here (n*n*8 + 16*n + small <= 64 KiB)
constexpr int LP = 65;              // lane form: LDS stride of one element across the 64 lanes (odd: the staging stores spread over banks)

enum Op { OP_GETRF = 0, OP_GETRS, OP_GESV, OP_SYTRF, OP_SYTRS, OP_SYSV };
constexpr bool op_fact(int op) { return op == OP_GETRF || op == OP_GESV || op == OP_SYTRF || op == OP_SYSV; }
constexpr bool op_solve(int op) { return op == OP_GETRS || op == OP_GESV || op == OP_SYTRS || op == OP_SYSV; }
constexpr int op_kind(int op) { return op >= OP_SYTRF ? 1 : 0; }   // 0: LU, 1: Bunch-Kaufman

struct BParams {
    double* A; int* ipiv; int* info; double* b;
    int n; long long count; int lhs_stride;
};

__device__ inline void dswap(double& x, double& y) { const double t = x; x = y; y = t; }

// ---------------------------------------------------------------------------------------------------------------------
// sequential routines (one lane, one problem).  Element (i, j) of the matrix (0-based) is a[(i + n*j)*EA], pivot i is
// pv[i*EA], entry i of the right-hand side x[i*EX].
// ---------------------------------------------------------------------------------------------------------------------
template <int EA>
__device__ inline int seq_getf2(double* a, int* pv, int n) {
#define M_(i, j) a[((i) + n * (j)) * EA]
    int info = 0;
    for (int j = 0; j < n; ++j) {
        int p = j; double best = fabs(M_(j, j));
        for (int i = j + 1; i < n; ++i) { const double v = fabs(M_(i, j)); if (v > best) { best = v; p = i; } }
        pv[j * EA] = p + 1;
        const double d = M_(p, j);
        if (d != 0.0) {
            if (p != j)
                for (int c = 0; c < n; ++c) dswap(M_(j, c), M_(p, c));
            if (fabs(d) >= DBL_MIN) { const double r = 1.0 / d; for (int i = j + 1; i < n; ++i) M_(i, j) *= r; }
            else for (int i = j + 1; i < n; ++i) M_(i, j) /= d;
        } else if (!info) {
            info = j + 1;
        }
        for (int c = j + 1; c < n; ++c) {
            const double u = M_(j, c);
            for (int i = j + 1; i < n; ++i) M_(i, c) -= M_(i, j) * u;
        }
    }
    return info;
#undef M_
}

template <int EA, int EX>
__device__ inline void seq_getrs(const double* a, const int* pv, double* x, int n) {
#define M_(i, j) a[((i) + n * (j)) * EA]
#define X_(i) x[(i) * EX]
    for (int i = 0; i < n; ++i) { const int p = pv[i * EA] - 1; if (p != i) dswap(X_(i), X_(p)); }
    for (int j = 0; j < n; ++j) {
        const double xj = X_(j);
        if (xj != 0.0) for (int i = j + 1; i < n; ++i) X_(i) -= xj * M_(i, j);
    }
    for (int j = n - 1; j >= 0; --j) {
        if (X_(j) != 0.0) {
            const double xj = X_(j) / M_(j, j);
            X_(j) = xj;
            for (int i = 0; i < j; ++i) X_(i) -= xj * M_(i, j);
        }
    }
#undef X_
#undef M_
}

// dsytf2, uplo = 'U' (1-based indices inside, as in the LAPACK routine)
template <int EA>
__device__ inline int seq_sytf2(double* a, int* pv, int n) {
#define U_(i, j) a[((i) - 1 + n * ((j) - 1)) * EA]
    const double alpha = (1.0 + sqrt(17.0)) / 8.0;
    int info = 0;
    int k = n;
    while (k >= 1) {
        int kstep = 1, kp = k;
        const double absakk = fabs(U_(k, k));
        int imax = 1; double colmax = 0.0;
        if (k > 1) {
            colmax = fabs(U_(1, k));
            for (int i = 2; i <= k - 1; ++i) { const double v = fabs(U_(i, k)); if (v > colmax) { colmax = v; imax = i; } }
        }
        if ((absakk > colmax ? absakk : colmax) == 0.0 || isnan(absakk)) {
            if (!info) info = k;
            kp = k;
        } else {
            if (absakk >= alpha * colmax) {
                kp = k;
            } else {
                double rowmax = fabs(U_(imax, imax + 1));
                for (int j = imax + 2; j <= k; ++j) { const double v = fabs(U_(imax, j)); if (v > rowmax) rowmax = v; }
                if (imax > 1) {
                    double cm = fabs(U_(1, imax));
                    for (int i = 2; i <= imax - 1; ++i) { const double v = fabs(U_(i, imax)); if (v > cm) cm = v; }
                    if (cm > rowmax) rowmax = cm;
                }
                if (absakk >= alpha * colmax * (colmax / rowmax)) kp = k;
                else if (fabs(U_(imax, imax)) >= alpha * rowmax) kp = imax;
                else { kp = imax; kstep = 2; }
            }
            const int kk = k - kstep + 1;
            if (kp != kk) {
                for (int i = 1; i <= kp - 1; ++i) dswap(U_(i, kk), U_(i, kp));
                for (int j = kp + 1; j <= kk - 1; ++j) dswap(U_(j, kk), U_(kp, j));
                dswap(U_(kk, kk), U_(kp, kp));
                if (kstep == 2) dswap(U_(k - 1, k), U_(kp, k));
            }
            if (kstep == 1) {
                const double r1 = 1.0 / U_(k, k);
                for (int j = 1; j <= k - 1; ++j) {
                    const double xj = U_(j, k);
                    if (xj != 0.0) { const double t = -r1 * xj; for (int i = 1; i <= j; ++i) U_(i, j) += U_(i, k) * t; }
                }
                for (int i = 1; i <= k - 1; ++i) U_(i, k) *= r1;
            } else if (k > 2) {
                double d12 = U_(k - 1, k);
                const double d22 = U_(k - 1, k - 1) / d12;
                const double d11 = U_(k, k) / d12;
                const double t = 1.0 / (d11 * d22 - 1.0);
                d12 = t / d12;
                for (int j = k - 2; j >= 1; --j) {
                    const double wkm1 = d12 * (d11 * U_(j, k - 1) - U_(j, k));
                    const double wk = d12 * (d22 * U_(j, k) - U_(j, k - 1));
                    for (int i = j; i >= 1; --i) U_(i, j) = U_(i, j) - U_(i, k) * wk - U_(i, k - 1) * wkm1;
                    U_(j, k) = wk;
                    U_(j, k - 1) = wkm1;
                }
            }
        }
        if (kstep == 1) pv[(k - 1) * EA] = kp;
        else { pv[(k - 1) * EA] = -kp; pv[(k - 2) * EA] = -kp; }
        k -= kstep;
    }
    return info;
#undef U_
}

// dsytrs, uplo = 'U', one right-hand side
template <int EA, int EX>
__device__ inline void seq_sytrs(const double* a, const int* pv, double* x, int n) {
#define U_(i, j) a[((i) - 1 + n * ((j) - 1)) * EA]
#define X_(i) x[((i) - 1) * EX]
#define P_(i) pv[((i) - 1) * EA]
    int k = n;
    while (k >= 1) {
        if (P_(k) > 0) {
            const int kp = P_(k);
            if (kp != k) dswap(X_(k), X_(kp));
            const double xk = X_(k);
            if (xk != 0.0) { const double t = -xk; for (int i = 1; i <= k - 1; ++i) X_(i) += U_(i, k) * t; }
            X_(k) *= 1.0 / U_(k, k);
            k -= 1;
        } else {
            const int kp = -P_(k);
            if (kp != k - 1) dswap(X_(k - 1), X_(kp));
            const double xk = X_(k), xkm1 = X_(k - 1);
            if (xk != 0.0) { const double t = -xk; for (int i = 1; i <= k - 2; ++i) X_(i) += U_(i, k) * t; }
            if (xkm1 != 0.0) { const double t = -xkm1; for (int i = 1; i <= k - 2; ++i) X_(i) += U_(i, k - 1) * t; }
            const double akm1k = U_(k - 1, k);
            const double akm1 = U_(k - 1, k - 1) / akm1k;
            const double ak = U_(k, k) / akm1k;
            const double denom = akm1 * ak - 1.0;
            const double bkm1 = xkm1 / akm1k, bk = xk / akm1k;
            X_(k - 1) = (ak * bkm1 - bk) / denom;
            X_(k) = (akm1 * bk - bkm1) / denom;
            k -= 2;
        }
    }
    k = 1;
    while (k <= n) {
        double s = 0.0;
        for (int i = 1; i <= k - 1; ++i) s += U_(i, k) * X_(i);
        if (P_(k) > 0) {
            X_(k) -= s;
            const int kp = P_(k);
            if (kp != k) dswap(X_(k), X_(kp));
            k += 1;
        } else {
            double s2 = 0.0;
            for (int i = 1; i <= k - 1; ++i) s2 += U_(i, k + 1) * X_(i);
            X_(k) -= s;
            X_(k + 1) -= s2;
            const int kp = -P_(k);
            if (kp != k) dswap(X_(k), X_(kp));
            k += 2;
        }
    }
#undef P_
#undef X_
#undef U_
}

// ---------------------------------------------------------------------------------------------------------------------
// LANE form: a wave of 64 problems, every problem one lane, the wave's matrices transposed into LDS
// ---------------------------------------------------------------------------------------------------------------------
template <int KIND, bool FACT, bool SOLVE>
__global__ __launch_bounds__(64) void lane_kernel(BParams p) {
    extern __shared__ double lds[];
    const int n = p.n, n2 = n * n, lane = threadIdx.x;
    const long long s0 = (long long)blockIdx.x * 64;
    const int ns = (int)(p.count - s0 < 64 ? p.count - s0 : 64);
    const bool shared = !FACT && p.lhs_stride == 0;               // one factor for every right-hand side
    double* sA = lds;
    double* sX = lds + (shared ? n2 : n2 * LP);
    int* sP = reinterpret_cast<int*>(sX + (SOLVE ? n * LP : 0));
    if (shared) {
        for (int t = lane; t < n2; t += 64) sA[t] = p.A[t];
        for (int t = lane; t < n; t += 64) sP[t] = p.ipiv[t];
    } else {
        const double* gA = p.A + s0 * n2;
        for (int t = lane; t < ns * n2; t += 64) { const int q = t / n2; sA[(t - q * n2) * LP + q] = gA[t]; }
        if (!FACT) {
            const int* gP = p.ipiv + s0 * n;
            for (int t = lane; t < ns * n; t += 64) { const int q = t / n; sP[(t - q * n) * LP + q] = gP[t]; }
        }
    }
    if (SOLVE) {
        const double* gb = p.b + s0 * n;
        for (int t = lane; t < ns * n; t += 64) { const int q = t / n; sX[(t - q * n) * LP + q] = gb[t]; }
    }
    __syncthreads();
    if (lane < ns) {
        if (shared) {
            if (KIND == 0) seq_getrs<1, LP>(sA, sP, sX + lane, n);
            else seq_sytrs<1, LP>(sA, sP, sX + lane, n);
        } else {
            double* a = sA + lane; int* pv = sP + lane;
            int info = 0;
            if (FACT) {
                info = KIND == 0 ? seq_getf2<LP>(a, pv, n) : seq_sytf2<LP>(a, pv, n);
                if (p.info) p.info[s0 + lane] = info;
            }
            if (SOLVE && info == 0) {                             // dgesv / dsysv: a singular system keeps its b as it came
                if (KIND == 0) seq_getrs<LP, LP>(a, pv, sX + lane, n);
                else seq_sytrs<LP, LP>(a, pv, sX + lane, n);
            }
        }
    }
    __syncthreads();
    if (FACT) {
        double* gA = p.A + s0 * n2;
        for (int t = lane; t < ns * n2; t += 64) { const int q = t / n2; gA[t] = sA[(t - q * n2) * LP + q]; }
        int* gP = p.ipiv + s0 * n;
        for (int t = lane; t < ns * n; t += 64) { const int q = t / n; gP[t] = sP[(t - q * n) * LP + q]; }
    }
    if (SOLVE) {
        double* gb = p.b + s0 * n;
        for (int t = lane; t < ns * n; t += 64) { const int q = t / n; gb[t] = sX[(t - q * n) * LP + q]; }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// GROUP form: one workgroup of NT threads per problem
// ---------------------------------------------------------------------------------------------------------------------
// (v, i) of the largest v over the block, the smallest i among equal v (idamax: the first largest entry); every thread gets it
template <int NT>
__device__ inline void blk_argmax(double& v, int& i, double* rv, int* ri) {
    for (int o = 32; o >= 1; o >>= 1) {
        const double ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(i, o);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
    if (NT > 64) {
        const int w = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) { rv[w] = v; ri[w] = i; }
        __syncthreads();
        v = rv[0]; i = ri[0];
        for (int q = 1; q < NT / 64; ++q)
            if (rv[q] > v || (rv[q] == v && ri[q] < i)) { v = rv[q]; i = ri[q]; }
        __syncthreads();
    }
}

// sum over the block in a fixed order (the butterfly gives every lane the same bits); every thread gets it
template <int NT>
__device__ inline double blk_sum(double v, double* rv) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if (NT > 64) {
        const int w = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) rv[w] = v;
        __syncthreads();
        v = rv[0];
        for (int q = 1; q < NT / 64; ++q) v += rv[q];
        __syncthreads();
    }
    return v;
}

template <int NT>
__device__ int grp_getf2(double* a, int* pv, int n, double* rv, int* ri) {
    const int tid = threadIdx.x;
    int info = 0;
    for (int j = 0; j < n; ++j) {
        double v = -1.0; int p = INT_MAX;
        // idamax: nothing beats a NaN head (the key +inf, and the smallest index wins ties); a NaN further down never wins
        for (int i = j + tid; i < n; i += NT) {
            double t = fabs(a[i + (size_t)n * j]);
            if (i == j && isnan(t)) t = INFINITY;
            if (t > v) { v = t; p = i; }
        }
        blk_argmax<NT>(v, p, rv, ri);
        if (p == INT_MAX) p = j;
        if (tid == 0) pv[j] = p + 1;
        const double d = a[p + (size_t)n * j];
        if (NT > 64) __syncthreads();                             // every wave has read d before the rows move
        if (d != 0.0) {
            if (p != j)
                for (int c = tid; c < n; c += NT) dswap(a[j + (size_t)n * c], a[p + (size_t)n * c]);
            __syncthreads();
            if (fabs(d) >= DBL_MIN) { const double r = 1.0 / d; for (int i = j + 1 + tid; i < n; i += NT) a[i + (size_t)n * j] *= r; }
            else for (int i = j + 1 + tid; i < n; i += NT) a[i + (size_t)n * j] /= d;
        } else if (!info) {
            info = j + 1;
        }
        __syncthreads();
        const int m = n - j - 1;
        for (int e = tid; e < m * m; e += NT) {
            const int i = j + 1 + e % m, c = j + 1 + e / m;
            a[i + (size_t)n * c] -= a[i + (size_t)n * j] * a[j + (size_t)n * c];
        }
        __syncthreads();
    }
    return info;
}

// x (LDS, n entries) in, solution out in y (LDS); the factor is read where it lies (LDS or global)
template <int NT>
__device__ void grp_getrs(const double* a, const int* pv, double* x, double* y, int n) {
    const int tid = threadIdx.x;
    if (tid == 0)
        for (int i = 0; i < n; ++i) { const int p = pv[i] - 1; if (p != i) dswap(x[i], x[p]); }
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        const double xj = x[j];
        if (xj != 0.0) for (int i = j + 1 + tid; i < n; i += NT) x[i] -= xj * a[i + (size_t)n * j];
        __syncthreads();
    }
    for (int j = n - 1; j >= 0; --j) {
        double xj = x[j];
        if (xj != 0.0) {
            xj = xj / a[j + (size_t)n * j];
            for (int i = tid; i < j; i += NT) x[i] -= xj * a[i + (size_t)n * j];
        }
        if (tid == 0) y[j] = xj;
        __syncthreads();
    }
}

template <int NT>
__device__ int grp_sytf2(double* a, int* pv, int n, double* rv, int* ri) {
#define U_(i, j) a[((i) - 1) + (size_t)n * ((j) - 1)]
    const int tid = threadIdx.x;
    const double alpha = (1.0 + sqrt(17.0)) / 8.0;
    int info = 0;
    int k = n;
    while (k >= 1) {
        int kstep = 1, kp = k;
        const double absakk = fabs(U_(k, k));
        double colmax = -1.0; int imax = INT_MAX;
        for (int i = 1 + tid; i <= k - 1; i += NT) {              // idamax, NaN head as in grp_getf2
            double t = fabs(U_(i, k));
            if (i == 1 && isnan(t)) t = INFINITY;
            if (t > colmax) { colmax = t; imax = i; }
        }
        blk_argmax<NT>(colmax, imax, rv, ri);
        if (k == 1) colmax = 0.0;
        else { if (imax == INT_MAX) imax = 1; colmax = fabs(U_(imax, k)); }
        if ((absakk > colmax ? absakk : colmax) == 0.0 || isnan(absakk)) {
            if (!info) info = k;
            kp = k;
        } else {
            if (absakk >= alpha * colmax) {
                kp = k;
            } else {
                // largest off-diagonal |entry| of row / column imax inside the leading k x k block
                double rowmax = -1.0; int dummy = 0;
                for (int j = imax + 1 + tid; j <= k; j += NT) { const double t = fabs(U_(imax, j)); if (t > rowmax) rowmax = t; }
                for (int i = 1 + tid; i <= imax - 1; i += NT) { const double t = fabs(U_(i, imax)); if (t > rowmax) rowmax = t; }
                blk_argmax<NT>(rowmax, dummy, rv, ri);
                if (absakk >= alpha * colmax * (colmax / rowmax)) kp = k;
                else if (fabs(U_(imax, imax)) >= alpha * rowmax) kp = imax;
                else { kp = imax; kstep = 2; }
            }
            const int kk = k - kstep + 1;
            if (NT > 64) __syncthreads();                         // every wave has made the decision before the entries move
            if (kp != kk) {
                for (int i = 1 + tid; i <= kp - 1; i += NT) dswap(U_(i, kk), U_(i, kp));
                for (int j = kp + 1 + tid; j <= kk - 1; j += NT) dswap(U_(j, kk), U_(kp, j));
                if (tid == 0) {
                    dswap(U_(kk, kk), U_(kp, kp));
                    if (kstep == 2) dswap(U_(k - 1, k), U_(kp, k));
                }
            }
            __syncthreads();
            if (kstep == 1) {
                const double r1 = 1.0 / U_(k, k);
                const int m = k - 1;
                for (int e = tid; e < m * m; e += NT) {
                    const int i = 1 + e % m, j = 1 + e / m;
                    if (i > j) continue;
                    const double xj = U_(j, k);
                    if (xj != 0.0) U_(i, j) += U_(i, k) * (-r1 * xj);
                }
                __syncthreads();
                for (int i = 1 + tid; i <= k - 1; i += NT) U_(i, k) *= r1;
                __syncthreads();
            } else if (k > 2) {
                double d12 = U_(k - 1, k);
                const double d22 = U_(k - 1, k - 1) / d12;
                const double d11 = U_(k, k) / d12;
                const double t = 1.0 / (d11 * d22 - 1.0);
                d12 = t / d12;
                const int m = k - 2;
                for (int e = tid; e < m * m; e += NT) {
                    const int i = 1 + e % m, j = 1 + e / m;
                    if (i > j) continue;
                    const double wkm1 = d12 * (d11 * U_(j, k - 1) - U_(j, k));
                    const double wk = d12 * (d22 * U_(j, k) - U_(j, k - 1));
                    U_(i, j) = U_(i, j) - U_(i, k) * wk - U_(i, k - 1) * wkm1;
                }
                __syncthreads();
                for (int j = 1 + tid; j <= m; j += NT) {
                    const double wkm1 = d12 * (d11 * U_(j, k - 1) - U_(j, k));
                    const double wk = d12 * (d22 * U_(j, k) - U_(j, k - 1));
                    U_(j, k) = wk;
                    U_(j, k - 1) = wkm1;
                }
                __syncthreads();
            }
        }
        if (tid == 0) {
            if (kstep == 1) pv[k - 1] = kp;
            else { pv[k - 1] = -kp; pv[k - 2] = -kp; }
        }
        k -= kstep;
    }
    __syncthreads();
    return info;
#undef U_
}

template <int NT>
__device__ void grp_sytrs(const double* a, const int* pv, double* x, double* y, int n, double* rv) {
#define U_(i, j) a[((i) - 1) + (size_t)n * ((j) - 1)]
#define X_(i) x[(i) - 1]
    const int tid = threadIdx.x;
    int k = n;
    while (k >= 1) {
        const int pk = pv[k - 1];
        if (pk > 0) {
            if (tid == 0 && pk != k) dswap(X_(k), X_(pk));
            __syncthreads();
            const double xk = X_(k);
            if (xk != 0.0) { const double t = -xk; for (int i = 1 + tid; i <= k - 1; i += NT) X_(i) += U_(i, k) * t; }
            __syncthreads();
            if (tid == 0) X_(k) = xk * (1.0 / U_(k, k));
            k -= 1;
        } else {
            const int kp = -pk;
            if (tid == 0 && kp != k - 1) dswap(X_(k - 1), X_(kp));
            __syncthreads();
            const double xk = X_(k), xkm1 = X_(k - 1);
            for (int i = 1 + tid; i <= k - 2; i += NT) {
                if (xk != 0.0) X_(i) += U_(i, k) * (-xk);
                if (xkm1 != 0.0) X_(i) += U_(i, k - 1) * (-xkm1);
            }
            __syncthreads();
            if (tid == 0) {
                const double akm1k = U_(k - 1, k);
                const double akm1 = U_(k - 1, k - 1) / akm1k;
                const double ak = U_(k, k) / akm1k;
                const double denom = akm1 * ak - 1.0;
                const double bkm1 = xkm1 / akm1k, bk = xk / akm1k;
                X_(k - 1) = (ak * bkm1 - bk) / denom;
                X_(k) = (akm1 * bk - bkm1) / denom;
            }
            k -= 2;
        }
    }
    __syncthreads();
    k = 1;
    while (k <= n) {
        const int pk = pv[k - 1];
        double s = 0.0;
        for (int i = 1 + tid; i <= k - 1; i += NT) s += U_(i, k) * X_(i);
        s = blk_sum<NT>(s, rv);
        if (pk > 0) {
            if (tid == 0) { X_(k) -= s; if (pk != k) dswap(X_(k), X_(pk)); }
            __syncthreads();
            k += 1;
        } else {
            double s2 = 0.0;
            for (int i = 1 + tid; i <= k - 1; i += NT) s2 += U_(i, k + 1) * X_(i);
            s2 = blk_sum<NT>(s2, rv);
            if (tid == 0) {
                X_(k) -= s;
                X_(k + 1) -= s2;
                if (-pk != k) dswap(X_(k), X_(-pk));
            }
            __syncthreads();
            k += 2;
        }
    }
    for (int i = tid; i < n; i += NT) y[i] = x[i];
    __syncthreads();
#undef X_
#undef U_
}

template <int NT, int KIND, bool FACT, bool SOLVE, bool IN_LDS>
__global__ __launch_bounds__(NT) void group_kernel(BParams p) {
    extern __shared__ double lds[];
    const int n = p.n, tid = threadIdx.x;
    const size_t n2 = (size_t)n * n;
    const long long s = blockIdx.x;
    const long long l = s * p.lhs_stride;
    double* gA = p.A + (size_t)l * n2;
    int* gP = p.ipiv + (size_t)l * n;
    double* a = IN_LDS ? lds : gA;
    double* xs = IN_LDS ? lds + n2 : lds;
    double* ys = xs + n;
    double* rv = ys + n;
    int* ri = reinterpret_cast<int*>(rv + NT / 64);
    if (IN_LDS)
        for (size_t e = tid; e < n2; e += NT) a[e] = gA[e];
    if (SOLVE)
        for (int i = tid; i < n; i += NT) xs[i] = p.b[(size_t)s * n + i];
    __syncthreads();
    int info = 0;                                                 // uniform over the workgroup
    if (FACT) {
        info = KIND == 0 ? grp_getf2<NT>(a, gP, n, rv, ri) : grp_sytf2<NT>(a, gP, n, rv, ri);
        if (tid == 0 && p.info) p.info[s] = info;
        __syncthreads();
    }
    if (SOLVE && info == 0) {                                     // dgesv / dsysv: a singular system keeps its b as it came
        if (KIND == 0) grp_getrs<NT>(a, gP, xs, ys, n);
        else grp_sytrs<NT>(a, gP, xs, ys, n, rv);
        for (int i = tid; i < n; i += NT) p.b[(size_t)s * n + i] = ys[i];
    }
    if (IN_LDS && FACT)
        for (size_t e = tid; e < n2; e += NT) gA[e] = a[e];
}

__global__ void symmetrize_kernel(double* A, int n, long long count) {
    const long long n2 = (long long)n * n, total = n2 * count;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const long long k = e / n2;
        const int r = (int)(e - k * n2), i = r % n, j = r / n;
        if (i >= j) continue;                                     // strict upper triangle: each pair once
        double* M = A + k * n2;
        const double t = 0.5 * (M[i + (size_t)n * j] + M[j + (size_t)n * i]);
        M[i + (size_t)n * j] = t;
        M[j + (size_t)n * i] = t;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// dispatch
// ---------------------------------------------------------------------------------------------------------------------
template <int KIND, bool FACT, bool SOLVE>
static int launch_lane(const BParams& p, hipStream_t s) {
    const bool shared = !FACT && p.lhs_stride == 0;
    const int n = p.n, n2 = n * n;
    const size_t lds = (size_t)(shared ? n2 : n2 * LP) * 8 + (SOLVE ? (size_t)n * LP * 8 : 0) + (size_t)(shared ? n : n * LP) * 4;
    const long long blocks = (p.count + 63) / 64;
    hipLaunchKernelGGL((lane_kernel<KIND, FACT, SOLVE>), dim3((unsigned)blocks), dim3(64), lds, s, p);
    WLSQM_HIP_CHECK(hipGetLastError());
    return WLSQM_OK;
}

template <int NT, int KIND, bool FACT, bool SOLVE>
static int launch_group(const BParams& p, hipStream_t s) {
    const int n = p.n;
    const bool in_lds = FACT && n <= GROUP_LDS_NMAX;
    const size_t lds = (in_lds ? (size_t)n * n * 8 : 0) + (size_t)2 * n * 8 + (NT / 64) * 12;
    if (in_lds) hipLaunchKernelGGL((group_kernel<NT, KIND, FACT, SOLVE, FACT>), dim3((unsigned)p.count), dim3(NT), lds, s, p);
    else hipLaunchKernelGGL((group_kernel<NT, KIND, FACT, SOLVE, false>), dim3((unsigned)p.count), dim3(NT), lds, s, p);
    WLSQM_HIP_CHECK(hipGetLastError());
    return WLSQM_OK;
}

template <int KIND, bool FACT, bool SOLVE>
static int launch_form(const BParams& p, hipStream_t s) {
    if (p.n <= LANE_NMAX) return launch_lane<KIND, FACT, SOLVE>(p, s);
    if (p.n <= 32) return launch_group<64, KIND, FACT, SOLVE>(p, s);
    return launch_group<256, KIND, FACT, SOLVE>(p, s);
}

static int launch_op(int op, BParams p, hipStream_t s) {
    // launches of at most CH problems, so that blocks x threads stays below 2^31 work-items in every form: lane 2^24 / 64
    // per block x 64 threads, group of 64 2^24 x 64 = 2^30, group of 256 2^22 x 256 = 2^30 (2^24 x 256 would be 2^32,
    // past the 32-bit grid size of a dispatch)
    const long long CH = p.n > 32 ? 1LL << 22 : 1LL << 24;
    const long long count = p.count;
    for (long long c0 = 0; c0 < count; c0 += CH) {
        BParams q = p;
        q.count = count - c0 < CH ? count - c0 : CH;
        const size_t lhs0 = (size_t)(c0 * p.lhs_stride);
        q.A = p.A + lhs0 * p.n * p.n;
        q.ipiv = p.ipiv + lhs0 * p.n;
        q.info = p.info ? p.info + c0 : nullptr;
        q.b = p.b ? p.b + (size_t)c0 * p.n : nullptr;
        int rc;
        switch (op) {
            case OP_GETRF: rc = launch_form<0, true, false>(q, s); break;
            case OP_GETRS: rc = launch_form<0, false, true>(q, s); break;
            case OP_GESV: rc = launch_form<0, true, true>(q, s); break;
            case OP_SYTRF: rc = launch_form<1, true, false>(q, s); break;
            case OP_SYTRS: rc = launch_form<1, false, true>(q, s); break;
            default: rc = launch_form<1, true, true>(q, s); break;
        }
        if (rc != WLSQM_OK) return rc;
    }
    return WLSQM_OK;
}

static int validate(int op, int n, long long count, int lhs_stride, const void* A, const void* ipiv, const void* b) {
    if (n < 1) { set_error("n must be >= 1"); return WLSQM_EVALUE; }
    if (count < 0) { set_error("count must be >= 0"); return WLSQM_EVALUE; }
    if (lhs_stride != 0 && lhs_stride != 1) { set_error("lhs_stride must be 0 or 1"); return WLSQM_EVALUE; }
    if (!A || !ipiv || (op_solve(op) && !b)) { set_error("null array"); return WLSQM_EVALUE; }
    if ((long long)n * n > INT_MAX / 2) { set_error("n too large"); return WLSQM_EVALUE; }
    return WLSQM_OK;
}

static int device_op(int op, int n, long long count, int lhs_stride, double* A, int* ipiv, int* info, double* b, int device,
                     hipStream_t s) {
    int rc = validate(op, n, count, lhs_stride, A, ipiv, b);
    if (rc != WLSQM_OK) return rc;
    DeviceScope scope;
    if ((rc = scope.enter(device)) != WLSQM_OK) return rc;
    if (count == 0) return WLSQM_OK;
    BParams p{A, ipiv, info, b, n, count, op_fact(op) ? 1 : lhs_stride};
    return launch_op(op, p, s);
}

struct LapackHostCtx {
    Stager st;
    GrowBuf A, ipiv, info, b;
};
static LapackHostCtx* lapack_host_ctx(int device) {
    static thread_local LapackHostCtx* ctx[16] = {nullptr};
    if (device < 0 || device >= 16) return nullptr;
    if (!ctx[device]) ctx[device] = new LapackHostCtx();
    return ctx[device];
}

// host arrays: upload what the operation reads, run it on the device, download what it writes (pinned staging in chunks)
static int host_op(int op, int n, long long count, int lhs_stride, double* A, int* ipiv, int* info, double* b, int device) {
    int rc = validate(op, n, count, lhs_stride, A, ipiv, b);
    if (rc != WLSQM_OK) return rc;
    DeviceScope scope;
    if ((rc = scope.enter(device)) != WLSQM_OK) return rc;
    if (count == 0) return WLSQM_OK;
    LapackHostCtx* cx = lapack_host_ctx(device);
    if (!cx) { set_error("device ordinal out of range"); return WLSQM_ENODEVICE; }
    if ((rc = cx->st.ensure(device))) return rc;
    const bool fact = op_fact(op), solve = op_solve(op);
    const long long nlhs = fact ? count : (lhs_stride ? count : 1);
    const long long n2 = (long long)n * n;
    if ((rc = cx->A.need((size_t)nlhs * n2 * 8)) || (rc = cx->ipiv.need((size_t)nlhs * n * 4)) ||
        (fact && (rc = cx->info.need((size_t)count * 4))) || (solve && (rc = cx->b.need((size_t)count * n * 8))))
        return rc;
    hipStream_t s = nullptr;
    if ((rc = cx->st.upload_rows(cx->A.b.p, A, nlhs, n2, n2, 1, 1, 8, s))) return rc;
    if (!fact && (rc = cx->st.upload_rows(cx->ipiv.b.p, ipiv, nlhs, n, n, 1, 1, 4, s))) return rc;
    if (solve && (rc = cx->st.upload_rows(cx->b.b.p, b, count, n, n, 1, 1, 8, s))) return rc;
    BParams p{cx->A.as<double>(), cx->ipiv.as<int>(), fact ? cx->info.as<int>() : nullptr, solve ? cx->b.as<double>() : nullptr,
              n, count, fact ? 1 : lhs_stride};
    if ((rc = launch_op(op, p, s))) return rc;
    auto commit_to = [](void* dst, size_t row_bytes) {
        return [dst, row_bytes](int64_t r, const char* row) { std::memcpy(static_cast<char*>(dst) + (size_t)r * row_bytes, row, row_bytes); };
    };
    if (fact) {
        if ((rc = cx->st.download_rows(cx->A.b.p, nlhs, n2, 8, s, commit_to(A, (size_t)n2 * 8)))) return rc;
        if ((rc = cx->st.download_rows(cx->ipiv.b.p, nlhs, n, 4, s, commit_to(ipiv, (size_t)n * 4)))) return rc;
        if (info && (rc = cx->st.download_rows(cx->info.b.p, count, 1, 4, s, commit_to(info, 4)))) return rc;
    }
    if (solve && (rc = cx->st.download_rows(cx->b.b.p, count, n, 8, s, commit_to(b, (size_t)n * 8)))) return rc;
    WLSQM_HIP_CHECK(hipStreamSynchronize(s));
    return WLSQM_OK;
}

static int symmetrize_launch(double* A, int n, long long count, hipStream_t s) {
    const long long total = (long long)n * n * count;
    long long blocks = (total + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(symmetrize_kernel, dim3((unsigned)blocks), dim3(256), 0, s, A, n, count);
    WLSQM_HIP_CHECK(hipGetLastError());
    return WLSQM_OK;
}

}  // namespace lapack
}  // namespace wlsqm

using namespace wlsqm;
using namespace wlsqm::lapack;

extern "C" {

int wlsqm_hip_getrf_batched_device(int n, int64_t count, double* A, int32_t* ipiv, int32_t* info, int device, void* stream) {
    return device_op(OP_GETRF, n, count, 1, A, ipiv, info, nullptr, device, (hipStream_t)stream);
}
int wlsqm_hip_getrs_batched_device(int n, int64_t count, int lhs_stride, const double* A, const int32_t* ipiv, double* b,
                                   int device, void* stream) {
    return device_op(OP_GETRS, n, count, lhs_stride, const_cast<double*>(A), const_cast<int32_t*>(ipiv), nullptr, b, device,
                     (hipStream_t)stream);
}
int wlsqm_hip_gesv_batched_device(int n, int64_t count, double* A, int32_t* ipiv, int32_t* info, double* b, int device,
                                  void* stream) {
    return device_op(OP_GESV, n, count, 1, A, ipiv, info, b, device, (hipStream_t)stream);
}
int wlsqm_hip_sytrf_batched_device(int n, int64_t count, double* A, int32_t* ipiv, int32_t* info, int device, void* stream) {
    return device_op(OP_SYTRF, n, count, 1, A, ipiv, info, nullptr, device, (hipStream_t)stream);
}
int wlsqm_hip_sytrs_batched_device(int n, int64_t count, int lhs_stride, const double* A, const int32_t* ipiv, double* b,
                                   int device, void* stream) {
    return device_op(OP_SYTRS, n, count, lhs_stride, const_cast<double*>(A), const_cast<int32_t*>(ipiv), nullptr, b, device,
                     (hipStream_t)stream);
}
int wlsqm_hip_sysv_batched_device(int n, int64_t count, double* A, int32_t* ipiv, int32_t* info, double* b, int device,
                                  void* stream) {
    return device_op(OP_SYSV, n, count, 1, A, ipiv, info, b, device, (hipStream_t)stream);
}
int wlsqm_hip_symmetrize_batched_device(int n, int64_t count, double* A, int device, void* stream) {
    if (n < 1 || count < 0 || !A) { set_error(n < 1 ? "n must be >= 1" : count < 0 ? "count must be >= 0" : "null array"); return WLSQM_EVALUE; }
    DeviceScope scope;
    int rc = scope.enter(device);
    if (rc != WLSQM_OK || count == 0) return rc;
    return symmetrize_launch(A, n, count, (hipStream_t)stream);
}

int wlsqm_hip_getrf_batched_host(int n, int64_t count, double* A, int32_t* ipiv, int32_t* info, int device) {
    return host_op(OP_GETRF, n, count, 1, A, ipiv, info, nullptr, device);
}
int wlsqm_hip_getrs_batched_host(int n, int64_t count, int lhs_stride, const double* A, const int32_t* ipiv, double* b, int device) {
    return host_op(OP_GETRS, n, count, lhs_stride, const_cast<double*>(A), const_cast<int32_t*>(ipiv), nullptr, b, device);
}
int wlsqm_hip_gesv_batched_host(int n, int64_t count, double* A, int32_t* ipiv, int32_t* info, double* b, int device) {
    return host_op(OP_GESV, n, count, 1, A, ipiv, info, b, device);
}
int wlsqm_hip_sytrf_batched_host(int n, int64_t count, double* A, int32_t* ipiv, int32_t* info, int device) {
    return host_op(OP_SYTRF, n, count, 1, A, ipiv, info, nullptr, device);
}
int wlsqm_hip_sytrs_batched_host(int n, int64_t count, int lhs_stride, const double* A, const int32_t* ipiv, double* b, int device) {
    return host_op(OP_SYTRS, n, count, lhs_stride, const_cast<double*>(A), const_cast<int32_t*>(ipiv), nullptr, b, device);
}
int wlsqm_hip_sysv_batched_host(int n, int64_t count, double* A, int32_t* ipiv, int32_t* info, double* b, int device) {
    return host_op(OP_SYSV, n, count, 1, A, ipiv, info, b, device);
}
int wlsqm_hip_symmetrize_batched_host(int n, int64_t count, double* A, int device) {
    if (n < 1 || count < 0 || !A) { set_error(n < 1 ? "n must be >= 1" : count < 0 ? "count must be >= 0" : "null array"); return WLSQM_EVALUE; }
    DeviceScope scope;
    int rc = scope.enter(device);
    if (rc != WLSQM_OK || count == 0) return rc;
    LapackHostCtx* cx = lapack_host_ctx(device);
    if (!cx) { set_error("device ordinal out of range"); return WLSQM_ENODEVICE; }
    const long long n2 = (long long)n * n;
    if ((rc = cx->st.ensure(device)) || (rc = cx->A.need((size_t)count * n2 * 8))) return rc;
    hipStream_t s = nullptr;
    if ((rc = cx->st.upload_rows(cx->A.b.p, A, count, n2, n2, 1, 1, 8, s))) return rc;
    if ((rc = symmetrize_launch(cx->A.as<double>(), n, count, s))) return rc;
    if ((rc = cx->st.download_rows(cx->A.b.p, count, n2, 8, s, [A, n2](int64_t r, const char* row) {
             std::memcpy(A + (size_t)r * n2, row, (size_t)n2 * 8); })))
        return rc;
    WLSQM_HIP_CHECK(hipStreamSynchronize(s));
    return WLSQM_OK;
}

}  // extern "C"
