// stencil.hip — stencil operators: the product of a sparse matrix in sliced ELLPACK, one slice per wavefront ("SELL-64", the layout is
// stated in include/wlsqm_hip.h), with R stacked vectors, for nop value planes that share one column array.
//
// One wave per slice, one lane per row, four slices per workgroup.  The loop over the entries e < width[s] is wave-uniform; a lane whose
// row has ended is switched off by predicate (its padding is neither loaded nor multiplied: NaN there, or in X where no live entry
// points, cannot leak).  Operators and fields go in register blocks of at most 4 x 4 accumulators: one load of `col` and one gather of
// X per field serve every operator of the block.  Each accumulator is summed in entry order with fma, so the bits of a result depend on
// the structure and the inputs alone (not on the block sizes, the unroll or the launch).  The entry loop is unrolled so that a lane has
// UNROLL gathers in flight; the gathers rely on L2 (Morton-ordered points), as the index-based fit kernels do.  No LDS.
#include "wlsqm_dispatch.hpp"

#pragma clang fp contract(off)      // a * b + c below is two roundings; the fused sums are __builtin_fma

namespace wlsqm {

struct SellArgs {
    long long nrows;
    const int32_t* len; const int32_t* width; const long long* soff;
    const int32_t* col; const double* val; long long val_stride_op;
    int nop; int R;
    const double* X; long long sx_f, sx_p;
    double* Y; long long sy_f, sy_o, sy_i;
    double alpha, beta;
};

constexpr int SELL_BLOCK = 4;       // accumulators per axis of a register block

// One register block of one row: operators o0 .. o0 + no - 1 and fields r0 .. r0 + nr - 1 (no <= NO, nr <= NR; both wave-uniform).
// `at` is the slice's entry offset plus the lane, `wid` the slice's width, `n` this lane's live entries (0 for a lane without a row).
template <int NO, int NR>
__device__ __forceinline__ void sell_block(const SellArgs& a, long long at, int wid, int n, long long row, int o0, int no, int r0, int nr) {
    constexpr int UNROLL = NO * NR <= 4 ? 8 : 4;
    double acc[NO][NR];
#pragma unroll
    for (int o = 0; o < NO; ++o)
#pragma unroll
        for (int r = 0; r < NR; ++r) acc[o][r] = 0.0;
    const int32_t* col = a.col + at;
    const double* val = a.val + (long long)o0 * a.val_stride_op + at;
    const double* X = a.X + (long long)r0 * a.sx_f;
    for (int e = 0; e < wid; e += UNROLL) {                  // wave-uniform
        if (e + UNROLL <= n) {
            // every entry of the step is live in this lane: all loads first, then the sums in entry order
            double x[UNROLL][NR], v[UNROLL][NO];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const long long c = col[64LL * (e + u)];
#pragma unroll
                for (int r = 0; r < NR; ++r) if (r < nr) x[u][r] = X[r * a.sx_f + c * a.sx_p];
#pragma unroll
                for (int o = 0; o < NO; ++o) if (o < no) v[u][o] = val[o * a.val_stride_op + 64LL * (e + u)];
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
#pragma unroll
                for (int o = 0; o < NO; ++o)
#pragma unroll
                    for (int r = 0; r < NR; ++r)
                        if (o < no && r < nr) acc[o][r] = __builtin_fma(v[u][o], x[u][r], acc[o][r]);
        } else {
            // the row ends inside this step (or has ended): entry by entry, under the lane's predicate
            for (int u = 0; u < UNROLL && e + u < n; ++u) {
                const long long c = col[64LL * (e + u)];
                double x[NR];
#pragma unroll
                for (int r = 0; r < NR; ++r) if (r < nr) x[r] = X[r * a.sx_f + c * a.sx_p];
#pragma unroll
                for (int o = 0; o < NO; ++o) {
                    if (o < no) {
                        const double v = val[o * a.val_stride_op + 64LL * (e + u)];
#pragma unroll
                        for (int r = 0; r < NR; ++r) if (r < nr) acc[o][r] = __builtin_fma(v, x[r], acc[o][r]);
                    }
                }
            }
        }
    }
    if (row >= a.nrows) return;
    double* Y = a.Y + (long long)r0 * a.sy_f + (long long)o0 * a.sy_o + row * a.sy_i;
#pragma unroll
    for (int o = 0; o < NO; ++o)
#pragma unroll
        for (int r = 0; r < NR; ++r)
            if (o < no && r < nr) {
                double* y = Y + r * a.sy_f + o * a.sy_o;
                // beta == 0 does not read Y (a NaN there must not leak)
                *y = a.beta == 0.0 ? a.alpha * acc[o][r] : __builtin_fma(a.alpha, acc[o][r], a.beta * *y);
            }
}

// NO, NR: the block sizes, min(nop, 4) and min(R, 4) of the launch.  Larger counts loop over the blocks; the last block of an axis may be
// narrower (the `no`, `nr` of sell_block).
template <int NO, int NR>
__global__ void __launch_bounds__(256) sell_apply_kernel(const SellArgs a) {
    const int lane = threadIdx.x & 63;
    const long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long row = s * 64 + lane;
    if (s * 64 >= a.nrows) return;                           // wave-uniform
    const int wid = __builtin_amdgcn_readfirstlane(a.width[s]);
    const long long at = a.soff[s] + lane;
    int n = row < a.nrows ? a.len[row] : 0;
    n = n < wid ? n : wid;
    for (int o0 = 0; o0 < a.nop; o0 += NO) {
        const int no = a.nop - o0 < NO ? a.nop - o0 : NO;
        for (int r0 = 0; r0 < a.R; r0 += NR) {
            const int nr = a.R - r0 < NR ? a.R - r0 : NR;
            sell_block<NO, NR>(a, at, wid, n, row, o0, no, r0, nr);
        }
    }
}

template <int NO>
static void sell_launch_fields(const SellArgs& a, dim3 grid, hipStream_t stream) {
    switch (a.R < SELL_BLOCK ? a.R : SELL_BLOCK) {
        case 1: hipLaunchKernelGGL((sell_apply_kernel<NO, 1>), grid, dim3(256), 0, stream, a); break;
        case 2: hipLaunchKernelGGL((sell_apply_kernel<NO, 2>), grid, dim3(256), 0, stream, a); break;
        case 3: hipLaunchKernelGGL((sell_apply_kernel<NO, 3>), grid, dim3(256), 0, stream, a); break;
        default: hipLaunchKernelGGL((sell_apply_kernel<NO, 4>), grid, dim3(256), 0, stream, a); break;
    }
}

static int sell_launch(const SellArgs& a, hipStream_t stream) {
    const long long nslices = (a.nrows + 63) / 64;
    const dim3 grid((unsigned)((nslices + 3) / 4));
    switch (a.nop < SELL_BLOCK ? a.nop : SELL_BLOCK) {
        case 1: sell_launch_fields<1>(a, grid, stream); break;
        case 2: sell_launch_fields<2>(a, grid, stream); break;
        case 3: sell_launch_fields<3>(a, grid, stream); break;
        default: sell_launch_fields<4>(a, grid, stream); break;
    }
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("stencil-apply");
    return WLSQM_OK;
}

// out[o][dest[e]] = in[o][src[e]] for e < n: the values of the transposed matrix from those of the forward one (or any other
// rearrangement of the live entries), one (dest, src) pair for all planes.  Padding is named by no pair: neither read nor written.
__global__ void __launch_bounds__(256) sell_permute_kernel(long long n, const int32_t* dest, const int32_t* src, const double* in,
                                                           long long in_stride_op, double* out, long long out_stride_op, int nop) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const long long d = dest[e], s = src[e];
    for (int o = 0; o < nop; ++o) out[o * out_stride_op + d] = in[o * in_stride_op + s];
}

}  // namespace wlsqm

using namespace wlsqm;

extern "C" {

int wlsqm_hip_sell_apply_device(int64_t nrows, int64_t nslices, const int32_t* len, const int32_t* width, const int64_t* soff,
                                const int32_t* col, const double* val, int64_t val_stride_op, int nop,
                                int64_t R, const double* X, int64_t x_stride_field, int64_t x_stride_point,
                                double* Y, int64_t y_stride_field, int64_t y_stride_op, int64_t y_stride_row,
                                double alpha, double beta, int device, void* stream) {
    if (nop < 1) { set_error("sell_apply: nop must be >= 1"); return WLSQM_EVALUE; }
    if (R < 1 || R > INT32_MAX) { set_error("sell_apply: R must be >= 1"); return WLSQM_EVALUE; }
    if (nrows < 0 || nslices < 0 || nrows > 64 * nslices) {
        set_error("sell_apply: nrows is beyond the 64 * nslices rows that soff covers");
        return WLSQM_EVALUE;
    }
    if (nrows > 0 && (!len || !width || !soff || !col || !val || !X || !Y)) { set_error("null array"); return WLSQM_EVALUE; }
    DeviceScope scope;
    const int rc = scope.enter(device);
    if (rc != WLSQM_OK || nrows == 0) return rc;
    SellArgs a;
    a.nrows = nrows;
    a.len = len; a.width = width; a.soff = reinterpret_cast<const long long*>(soff);
    a.col = col; a.val = val; a.val_stride_op = val_stride_op;
    a.nop = nop; a.R = (int)R;
    a.X = X; a.sx_f = x_stride_field; a.sx_p = x_stride_point;
    a.Y = Y; a.sy_f = y_stride_field; a.sy_o = y_stride_op; a.sy_i = y_stride_row;
    a.alpha = alpha; a.beta = beta;
    return sell_launch(a, (hipStream_t)stream);
}

int wlsqm_hip_sell_permute_device(int64_t n, const int32_t* dest, const int32_t* src, const double* in, int64_t in_stride_op,
                                  double* out, int64_t out_stride_op, int nop, int device, void* stream) {
    if (nop < 1) { set_error("sell_permute: nop must be >= 1"); return WLSQM_EVALUE; }
    if (n < 0 || (n + 255) / 256 > 0x7fffffffLL) { set_error("sell_permute: n must be 0 .. 2^39"); return WLSQM_EVALUE; }
    if (n > 0 && (!dest || !src || !in || !out)) { set_error("null array"); return WLSQM_EVALUE; }
    DeviceScope scope;
    const int rc = scope.enter(device);
    if (rc != WLSQM_OK || n == 0) return rc;
    hipLaunchKernelGGL(sell_permute_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (long long)n, dest, src, in,
                       (long long)in_stride_op, out, (long long)out_stride_op, nop);
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("stencil-permute");
    return WLSQM_OK;
}

}  // extern "C"
