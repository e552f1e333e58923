// wlsqm_grid.hpp — the uniform grid over a device-resident cloud that the searches of knn.hip walk, shared with interp_plan.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "wlsqm_internal.hpp"

namespace wlsqm {

// order-preserving map double -> uint64 and back: what the bounding-box kernel's atomic min / max compare
__device__ __forceinline__ unsigned long long key_of(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
inline double value_of(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double v; memcpy(&v, &u, 8); return v;
}

// Bounding box of S[n, dim] (knn.hip; shared with order.hip): mm[m] = the least key_of over axis m, mm[3 + m] the greatest, met by atomics
// on what the caller has set to ~0 and 0.  A NaN wins either way, so that it is reported.  Any grid of 256-lane workgroups; the host stub
// that a launch from another translation unit goes through is the one knn.hip's unit registers (one library, no relocatable device code).
__global__ __launch_bounds__(256) void knn_bbox_kernel(const double* __restrict__ S, long long n, int dim, unsigned long long* mm /*[2][3]*/);

struct KnnGrid {
    double lo[3], inv_cell[3], cell[3];
    double sliver[3];      // the stop rule's margin on a cell boundary (knn.hip, head comment): max(1e-9, 2^-48 g) cell
    int g[3];
    int dim;
};

// Cell number of x on axis m, clamped to the grid IN DOUBLE: a query far outside the box has a quotient beyond int's range, which the
// conversion must never see, and a NaN compares false twice and lands in cell 0.  Monotone in x (every step is a monotone rounding).
__device__ __forceinline__ int cell_coord(double x, const KnnGrid& G, int m) {
    const double t = (x - G.lo[m]) * G.inv_cell[m];
    return t >= (double)G.g[m] ? G.g[m] - 1 : (t > 0.0 ? (int)t : 0);
}

// Uniform grid over a device-resident cloud: bounding box, cells of ~4 points, points sorted by cell (knn.hip).  Cell c holds the
// sorted positions d_start[c] .. d_start[c + 1] - 1; d_perm[pos] is the point's number and d_Ss[pos] its coordinates.  The sort
// is stable, so the points of one cell come in ascending number.  The shape (g, cell) is wlsqm_hip_grid_shape_host's (knn.hip), which
// also rejects a box with a non-finite bound or whose squared diagonal overflows.
struct GridIndex {
    KnnGrid G{};
    long long ncells = 1;
    DevBuf d_perm, d_start, d_Ss;
    int build(int dimension, int64_t npoints, const double* S, hipStream_t s);
};

}  // namespace wlsqm
