// The softmax of one row of C <= KC logits held in registers, as the cross entropy (loss.hip) and the Lovasz-Softmax loss (lovasz.hip)
// both form it: where the row begins in a class-strided [B, C, inner] tensor, its load, and d_c = x_c - max, log sum_c exp(d_c).
// The callers finish it themselves: p_c = expf(d_c - log sum).
//
// This header is compiled once with floating-point contraction on (loss.hip) and once with it off (lovasz.hip), and both must get the
// same bits: no function here holds a floating-point multiply that feeds an add (the only products are integer addresses).  Keep it so.
#pragma once
#include "pn2_common.h"

// first element of row r = b * inner + n of a [B, C, inner] tensor: neighbouring lanes read neighbouring n
__device__ __forceinline__ int64_t pn2_class_strided_base(int64_t r, int64_t inner, int C) {
    const int64_t b = r / inner;
    return b * C * inner + (r - b * inner);
}

// v[c] = row[c * step] for c < C: step 1 for a row-major row, `inner` for a class-strided one
template <int KC>
__device__ __forceinline__ void pn2_load_row_strided(const float *__restrict__ row, int64_t step, int C, float (&v)[KC]) {
#pragma unroll
    for (int c = 0; c < KC; ++c)
        if (c < C) v[c] = row[c * step];
}

// v <- v - max(v) over the C leading entries; returns log sum exp(v) (four interleaved partial sums: the tree shape of ATen's
// own row sum, see log_softmax_bwd_kernel)
template <int KC>
__device__ __forceinline__ float pn2_center_logsum(int C, float (&v)[KC]) {
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < KC; ++c)
        if (c < C) m = fmaxf(m, v[c]);
    float s4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < KC; ++c)
        if (c < C) { v[c] -= m; s4[c & 3] += expf(v[c]); }
    return logf((s4[0] + s4[1]) + (s4[2] + s4[3]));
}
