// The rigid map p = [R | t] s with T row major, in ONE place (icp.hip, corr_ransac.hip): the rounding registration.transform_points
// documents.  The callers are built with -ffp-contract=off: every term is a separate fp64 rounding.
#pragma once

// component ROW (0, 1, 2) of p
template <int ROW>
__device__ __forceinline__ double pn2_rigid_apply(const double (&T)[12], double x, double y, double z) {
    static_assert(ROW >= 0 && ROW < 3, "x, y or z");
    return ((T[4 * ROW] * x + T[4 * ROW + 1] * y) + T[4 * ROW + 2] * z) + T[4 * ROW + 3];
}
