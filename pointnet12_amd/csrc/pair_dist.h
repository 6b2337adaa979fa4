// The pair distance of the reference in its exact fp32 form (pinned in oracle/pn2_oracle.c), shared by geometry.hip and knn.hip.
// Both files are COMPILED WITH -ffp-contract=off: every fused step is an explicit __builtin_fmaf and nothing else may contract.
//   dot = fma(az,bz, fma(ay,by, ax*bx)); n(p) = ((x*x + y*y) + z*z);  d = ((-2*dot) + n(query)) + n(candidate)
#pragma once

namespace {

__device__ __forceinline__ float sq_norm3(float x, float y, float z) {
    float xx = x * x, yy = y * y, zz = z * z;
    return (xx + yy) + zz;
}

__device__ __forceinline__ float pair_dist(float qx, float qy, float qz, float nq, float px, float py, float pz,
                                           float np) {
    float dot = qx * px;
    dot = __builtin_fmaf(qy, py, dot);
    dot = __builtin_fmaf(qz, pz, dot);
    float d = -2.0f * dot;
    d = d + nq;
    d = d + np;
    return d;
}

}  // namespace
