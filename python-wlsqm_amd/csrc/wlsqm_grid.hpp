// wlsqm_grid.hpp — the uniform grid over a device-resident cloud that the searches of knn.hip walk, shared with interp_plan.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wlsqm_internal.hpp"

namespace wlsqm {

struct KnnGrid {
    double lo[3], inv_cell[3], cell[3];
    int g[3];
    int dim;
};

__device__ __forceinline__ int cell_coord(double x, const KnnGrid& G, int m) {
    int c = (int)((x - G.lo[m]) * G.inv_cell[m]);
    return c < 0 ? 0 : (c >= G.g[m] ? G.g[m] - 1 : c);
}

// Uniform grid over a device-resident cloud: bounding box, cells of ~4 points, points sorted by cell (knn.hip).  Cell c holds the
// sorted positions d_start[c] .. d_start[c + 1] - 1; d_perm[pos] is the point's number and d_Ss[pos] its coordinates.  The sort
// is stable, so the points of one cell come in ascending number.
struct GridIndex {
    KnnGrid G{};
    long long ncells = 1;
    DevBuf d_perm, d_start, d_Ss;
    int build(int dimension, int64_t npoints, const double* S, hipStream_t s);
};

}  // namespace wlsqm
