// The cell rule of the voxel grid (include/pn2.h), in ONE place: voxel.hip keys every row by it, and voxel_cluster.hip recomputes the
// cell of each voxel's representative row to find its neighbours -- the two must agree to the bit.  Both files are built with
// -ffp-contract=off: q = floor(((double)p - origin) / voxel) is two separately rounded fp64 operations.
#pragma once
#include <cmath>
#include "pn2_common.h"

struct Grid {
    double origin[3], voxel[3];
};

// the caller's grid; false unless every origin is finite and every voxel edge finite and positive
static inline bool pn2_grid_from(const double *origin, const double *voxel, Grid &grid) {
    for (int a = 0; a < 3; ++a) {
        if (!(std::isfinite(origin[a]) && std::isfinite(voxel[a]) && voxel[a] > 0.0)) return false;
        grid.origin[a] = origin[a];
        grid.voxel[a] = voxel[a];
    }
    return true;
}

constexpr long long kCells = 1ll << 21;                             // biased cells per axis

// the cell of one coordinate, biased to [0, kCells); false: outside the grid (or not finite)
__device__ __forceinline__ bool cell_of(float p, double origin, double voxel, unsigned long long &biased) {
    const double q = floor(((double)p - origin) / voxel);
    if (!(q >= -1048576.0 && q < 1048576.0)) return false;
    biased = (unsigned long long)((long long)q + 1048576ll);
    return true;
}

// the key of a cell: 21 bits per axis, x in the high bits
__device__ __forceinline__ unsigned long long pn2_cell_key(unsigned long long cx, unsigned long long cy, unsigned long long cz) {
    return (cx << 42) | (cy << 21) | cz;
}

// the key of the cell that holds (x, y, z); false: outside the grid
__device__ __forceinline__ bool pn2_cell_key_of(float x, float y, float z, const Grid &grid, unsigned long long &key) {
    unsigned long long cx, cy, cz;
    if (!(cell_of(x, grid.origin[0], grid.voxel[0], cx) && cell_of(y, grid.origin[1], grid.voxel[1], cy) &&
          cell_of(z, grid.origin[2], grid.voxel[2], cz)))
        return false;
    key = pn2_cell_key(cx, cy, cz);
    return true;
}
