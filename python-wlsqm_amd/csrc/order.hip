// order.hip — put a device-resident cloud in Morton order, and renumber neighbour lists with it.
//
// The order, stated once (tests/_order_ref.py is the same statement in numpy; the two agree bit for bit).  Per axis lo = min, hi = max
// over the points, ext = hi - lo (one rounded subtraction).
//   dim 2, 3:  B = 31 (2D) or 21 (3D) bits per axis.  q = 0 where ext == 0, else q = min(floor(((x - lo) / ext) * 2^B), 2^B - 1): one
//              correctly rounded subtraction, one correctly rounded division and an exact scaling.  No product is followed by a sum, so
//              there is nothing a compiler could contract.  Bit b of axis m is bit b * dim + m of the key: non-negative int64, 62 or 63 bits.
//              Monotone per axis (every step is a monotone rounding) and unchanged when the cloud is scaled by a power of two.
//   dim 1:     exact.  u = bits(x + 0.0) as int64 (-0.0 becomes +0.0); key = u where u >= 0, else u ^ 0x7fffffffffffffff.  The signed order
//              of the keys is the order of the doubles.
//   perm = the stable ascending sort of the keys (ties go to the smaller old index): new position i holds old point perm[i], and
//   inverse[perm[i]] = i.
// Points outside the box (wlsqm_hip_spatial_keys_device places ANY points under a given box) clamp to its ends; a NaN coordinate gives the
// largest key of the dimension.
//
// Kernels: "order-keys" (one lane per point), hipcub's radix sort of (int64 key, int32 index) pairs, "order-inverse" (one lane per
// point) and "order-relabel" (one lane per slot of a neighbour list: out[i, k] = inverse[hoods[row_perm[i], k]]).  The bounding box is
// knn.hip's knn_bbox_kernel, so that the order and the searches see the same box.
#include <cfloat>
#include <cmath>
#include <cstdint>

#include <hipcub/hipcub.hpp>

#include "wlsqm_dispatch.hpp"
#include "wlsqm_grid.hpp"

namespace wlsqm {

struct OrderBox {
    double lo[3], hi[3], ext[3];
    int dim;
};

// 32 bits to the even positions of 64
__device__ __forceinline__ unsigned long long spread2(unsigned long long x) {
    x &= 0xffffffffull;
    x = (x | (x << 16)) & 0x0000ffff0000ffffull;
    x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
    x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}
// 21 bits to every third position of 63
__device__ __forceinline__ unsigned long long spread3(unsigned long long x) {
    x &= 0x1fffffull;
    x = (x | (x << 32)) & 0x001f00000000ffffull;
    x = (x | (x << 16)) & 0x001f0000ff0000ffull;
    x = (x | (x << 8)) & 0x100f00f00f00f00full;
    x = (x | (x << 4)) & 0x10c30c30c30c30c3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}

// The cell of x on one axis: min(floor(((x - lo) / ext) * 2^B), 2^B - 1), clamped IN DOUBLE (a point far outside the box has a quotient
// beyond any integer's range, which the conversion must never see; a NaN compares false twice and gives 0: the caller has set the key).
__device__ __forceinline__ unsigned long long order_cell(double x, double lo, double ext, double scale) {
    if (!(ext > 0.0)) return 0ull;
    const double d = x - lo;
    const double t = d / ext;
    const double u = t * scale;        // exact: a power of two (a subnormal t may round, to something below 1 all the same)
    return u >= scale ? (unsigned long long)scale - 1ull : (u > 0.0 ? (unsigned long long)u : 0ull);
}

__device__ __forceinline__ long long order_key1(double x) {
    const long long u = __double_as_longlong(x + 0.0);
    return u >= 0 ? u : (u ^ 0x7fffffffffffffffll);
}

// keys[i] of point i under the box; idx[i] = i when idx is given (the values of the sort)
__global__ __launch_bounds__(256) void order_keys_kernel(const double* __restrict__ X, long long n, OrderBox box,
                                                         long long* __restrict__ keys, int* __restrict__ idx) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    long long key;
    if (box.dim == 1) {
        const double x = X[i];
        // clamped to the box (the cloud's own points are inside it: nothing changes for them)
        key = x != x ? 0x7fffffffffffffffll : order_key1(x < box.lo[0] ? box.lo[0] : (x > box.hi[0] ? box.hi[0] : x));
    } else if (box.dim == 2) {
        const double x = X[2 * i], y = X[2 * i + 1];
        key = (x != x || y != y) ? 0x3fffffffffffffffll
                                 : (long long)(spread2(order_cell(x, box.lo[0], box.ext[0], 0x1p31)) |
                                               (spread2(order_cell(y, box.lo[1], box.ext[1], 0x1p31)) << 1));
    } else {
        const double x = X[3 * i], y = X[3 * i + 1], z = X[3 * i + 2];
        key = (x != x || y != y || z != z) ? 0x7fffffffffffffffll
                                           : (long long)(spread3(order_cell(x, box.lo[0], box.ext[0], 0x1p21)) |
                                                         (spread3(order_cell(y, box.lo[1], box.ext[1], 0x1p21)) << 1) |
                                                         (spread3(order_cell(z, box.lo[2], box.ext[2], 0x1p21)) << 2));
    }
    keys[i] = key;
    if (idx) idx[i] = (int)i;
}

// inverse[perm[i]] = i (perm is the sort's output: a permutation of 0 .. n - 1)
__global__ __launch_bounds__(256) void order_inverse_kernel(const int* __restrict__ perm, long long n, int* __restrict__ inverse) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) inverse[perm[i]] = (int)i;
}

// One lane per slot.  A workgroup owns `rows_per_block` whole rows (about 2048 slots; one row when K is larger) and walks their slots in
// memory order: the writes of a workgroup are one contiguous run, its reads one contiguous run per source row, and the row of a slot
// comes from a 32-bit quotient (t / K from a double product, corrected by at most one: t < 2^32 makes the product's error below 2^-20).
// The one gather is the 4-byte `inverse` table.  A live entry outside 0 .. npoints - 1 is never dereferenced: it is written as -1 and
// counted, and so is every slot of a row whose row_perm entry is no row.
__global__ __launch_bounds__(256) void order_relabel_kernel(long long ncases, unsigned K, unsigned rows_per_block, double inv_K,
                                                            const int* __restrict__ hoods, long long row_stride,
                                                            const int* __restrict__ nk, const int* __restrict__ row_perm,
                                                            const int* __restrict__ inverse, long long npoints,
                                                            const int* __restrict__ own, int* __restrict__ out, int* __restrict__ bad) {
    const long long row0 = (long long)blockIdx.x * rows_per_block;
    const long long left = ncases - row0;
    const unsigned rows = left < (long long)rows_per_block ? (unsigned)left : rows_per_block;
    const unsigned long long slots = (unsigned long long)rows * K;      // < 2^32: rows_per_block * K <= max(2048, K)
    int nbad = 0;
    for (unsigned long long t64 = threadIdx.x; t64 < slots; t64 += 256) {
        const unsigned t = (unsigned)t64;
        unsigned q = (unsigned)((double)t * inv_K);
        long long rem = (long long)t - (long long)q * K;
        if (rem < 0) { --q; rem += K; } else if (rem >= (long long)K) { ++q; rem -= K; }
        const long long i = row0 + q;
        const int k = (int)rem;
        long long r = row_perm ? (long long)row_perm[i] : i;
        int v;
        if (r < 0 || r >= ncases) {
            v = -1; ++nbad;
        } else if (nk && k >= nk[r]) {
            v = own ? own[i] : (int)i;
        } else {
            const long long p = hoods[r * row_stride + k];
            if (p < 0 || p >= npoints) { v = -1; ++nbad; } else v = inverse[p];
        }
        out[i * (long long)K + k] = v;
    }
    if (bad && nbad) atomicAdd(bad, nbad);
}

}  // namespace wlsqm

using namespace wlsqm;

static int order_box(int dimension, const double* lo, const double* hi, OrderBox* box) {
    *box = OrderBox{};
    box->dim = dimension;
    for (int m = 0; m < dimension; ++m) { box->lo[m] = lo[m]; box->hi[m] = hi[m]; box->ext[m] = hi[m] - lo[m]; }
    return WLSQM_OK;
}

static int launch_order_keys(const double* X, long long n, const OrderBox& box, long long* keys, int* idx, hipStream_t s) {
    hipLaunchKernelGGL(order_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, X, n, box, keys, idx);
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("order-keys");
    return WLSQM_OK;
}

extern "C" {

int wlsqm_hip_spatial_order_device(int dimension, int64_t npoints, const double* S, int64_t* keys_sorted, int32_t* perm,
                                   int32_t* inverse, double* box_out, int device, void* stream) {
    if (dimension < 1 || dimension > 3) { set_error("dimension must be 1, 2 or 3"); return WLSQM_EVALUE; }
    if (npoints < 1) { set_error("npoints must be >= 1"); return WLSQM_EVALUE; }
    if (npoints > 0x7fffffffLL) { set_error("at most 2^31 - 1 points"); return WLSQM_EVALUE; }
    if (!S || !perm || !inverse || !box_out) { set_error("null array"); return WLSQM_EVALUE; }
    DeviceScope scope; int rc = scope.enter(device);
    if (rc != WLSQM_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const long long n = npoints;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    // 1. bounding box (knn.hip's kernel: the order and the searches see the same box, and a NaN is reported by either)
    DevBuf d_mm;
    if ((rc = d_mm.alloc(6 * sizeof(unsigned long long)))) return rc;
    unsigned long long h_mm[6] = {~0ull, ~0ull, ~0ull, 0ull, 0ull, 0ull};
    WLSQM_HIP_CHECK(hipMemcpyAsync(d_mm.p, h_mm, sizeof(h_mm), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(knn_bbox_kernel, dim3(blocks < 1024u ? blocks : 1024u), dim3(256), 0, s, S, n, dimension,
                       d_mm.as<unsigned long long>());
    WLSQM_HIP_CHECK(hipGetLastError());
    WLSQM_HIP_CHECK(hipMemcpyAsync(h_mm, d_mm.p, sizeof(h_mm), hipMemcpyDeviceToHost, s));
    WLSQM_HIP_CHECK(hipStreamSynchronize(s));
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    for (int m = 0; m < dimension; ++m) { lo[m] = value_of(h_mm[m]); hi[m] = value_of(h_mm[3 + m]); }
    // the domain of the searches: finite coordinates, a box whose squared diagonal is representable
    int32_t g[3]; double cell[3];
    if ((rc = wlsqm_hip_grid_shape_host(dimension, npoints, lo, hi, g, cell))) return rc;
    for (int m = 0; m < 3; ++m) { box_out[m] = lo[m]; box_out[3 + m] = hi[m]; }
    OrderBox box;
    order_box(dimension, lo, hi, &box);

    // 2. keys, 3. the stable sort of (key, index), 4. the inverse
    DevBuf d_keys, d_keys2, d_idx, d_tmp;
    if ((rc = d_keys.alloc((size_t)n * 8)) || (rc = d_idx.alloc((size_t)n * 4))) return rc;
    if (!keys_sorted && (rc = d_keys2.alloc((size_t)n * 8))) return rc;
    long long* sorted = keys_sorted ? reinterpret_cast<long long*>(keys_sorted) : d_keys2.as<long long>();
    if ((rc = launch_order_keys(S, n, box, d_keys.as<long long>(), d_idx.as<int>(), s))) return rc;
    const int end_bit = dimension == 1 ? 64 : (dimension == 2 ? 62 : 63);
    size_t tmp_bytes = 0;
    WLSQM_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, d_keys.as<long long>(), sorted, d_idx.as<int>(), perm, (int)n,
                                                       0, end_bit, s));
    if ((rc = d_tmp.alloc(tmp_bytes ? tmp_bytes : 16))) return rc;
    WLSQM_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(d_tmp.p, tmp_bytes, d_keys.as<long long>(), sorted, d_idx.as<int>(), perm, (int)n,
                                                       0, end_bit, s));
    hipLaunchKernelGGL(order_inverse_kernel, dim3(blocks), dim3(256), 0, s, perm, n, inverse);
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("order-inverse");
    WLSQM_HIP_CHECK(hipStreamSynchronize(s));      // the sort's temporaries are freed on return
    return WLSQM_OK;
}

int wlsqm_hip_spatial_keys_device(int dimension, int64_t n, const double* X, const double* lo, const double* hi, int64_t* keys,
                                  int device, void* stream) {
    if (dimension < 1 || dimension > 3) { set_error("dimension must be 1, 2 or 3"); return WLSQM_EVALUE; }
    if (n < 0 || (n + 255) / 256 > 0x7fffffffLL) { set_error("spatial_keys: n must be 0 .. 2^39"); return WLSQM_EVALUE; }
    if (!lo || !hi || (n > 0 && (!X || !keys))) { set_error("null array"); return WLSQM_EVALUE; }
    for (int m = 0; m < dimension; ++m) {
        if (!(std::fabs(lo[m]) <= DBL_MAX) || !(std::fabs(hi[m]) <= DBL_MAX)) { set_error("non-finite coordinates"); return WLSQM_EVALUE; }
        if (hi[m] < lo[m]) { set_error("the box's upper bound is below its lower bound"); return WLSQM_EVALUE; }
    }
    DeviceScope scope; const int rc = scope.enter(device);
    if (rc != WLSQM_OK || n == 0) return rc;
    OrderBox box;
    order_box(dimension, lo, hi, &box);
    return launch_order_keys(X, n, box, reinterpret_cast<long long*>(keys), nullptr, (hipStream_t)stream);
}

int wlsqm_hip_relabel_hoods_device(int64_t ncases, int K, const int32_t* hoods, int64_t row_stride, const int32_t* nk,
                                   const int32_t* row_perm, const int32_t* inverse, int64_t npoints, const int32_t* own, int32_t* out,
                                   int32_t* bad, int device, void* stream) {
    if (ncases < 0 || K < 0 || npoints < 0 || npoints > 0x7fffffffLL) { set_error("relabel_hoods: ncases, K >= 0 and 0 <= npoints < 2^31"); return WLSQM_EVALUE; }
    if (row_stride < K) { set_error("relabel_hoods: row_stride must be >= K"); return WLSQM_EVALUE; }
    DeviceScope scope; const int rc = scope.enter(device);
    if (rc != WLSQM_OK || ncases == 0 || K == 0) return rc;
    if (!hoods || !inverse || !out) { set_error("null array"); return WLSQM_EVALUE; }
    const unsigned rows_per_block = (unsigned)K >= 2048u ? 1u : 2048u / (unsigned)K;
    const long long blocks = (ncases + rows_per_block - 1) / rows_per_block;
    if (blocks > 0x7fffffffLL) { set_error("relabel_hoods: too many rows for one launch"); return WLSQM_EVALUE; }
    hipLaunchKernelGGL(order_relabel_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (long long)ncases, (unsigned)K,
                       rows_per_block, 1.0 / (double)K, hoods, (long long)row_stride, nk, row_perm, inverse, (long long)npoints, own, out,
                       bad);
    WLSQM_HIP_CHECK(hipGetLastError());
    note_kernel("order-relabel");
    return WLSQM_OK;
}

}  // extern "C"
