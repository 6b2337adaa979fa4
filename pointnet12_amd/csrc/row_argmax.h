// The row arg-max of the segmentation kernels (metrics.hip: pn2_seg_confusion; view.hip: pn2_seg_predict), in ONE place.
// Contract (include/pn2.h): the index of the row's largest entry among its first C columns, the LOWEST index on equal values; a
// NaN counts as largest and the first NaN wins; a row of all -inf gives 0 -- what torch.max(dim)[1] and argmax return.
#pragma once
#include "pn2_common.h"

__device__ __forceinline__ bool pn2_beats(float v, float best) { return v > best || (v != v && best == best); }

// QUADS: the row is read as float4 quads (ld % 4 == 0 and a 16-byte aligned base: the quad that holds column C - 1 lies inside the
// row); columns c >= C of the last quad are read but never compared.  Otherwise one float at a time.
template <bool QUADS>
__device__ __forceinline__ int pn2_row_argmax(const float *__restrict__ row, int C, float &best) {
    int arg = 0;
    if (QUADS) {
        const float4 *row4 = reinterpret_cast<const float4 *>(row);
        float4 t = row4[0];
        best = t.x;
        if (1 < C && pn2_beats(t.y, best)) { best = t.y; arg = 1; }
        if (2 < C && pn2_beats(t.z, best)) { best = t.z; arg = 2; }
        if (3 < C && pn2_beats(t.w, best)) { best = t.w; arg = 3; }
        for (int c = 4; c < C; c += 4) {
            t = row4[c >> 2];                             // ld >= round4(C): the quad lies inside the row
            if (pn2_beats(t.x, best)) { best = t.x; arg = c; }
            if (c + 1 < C && pn2_beats(t.y, best)) { best = t.y; arg = c + 1; }
            if (c + 2 < C && pn2_beats(t.z, best)) { best = t.z; arg = c + 2; }
            if (c + 3 < C && pn2_beats(t.w, best)) { best = t.w; arg = c + 3; }
        }
    } else {
        best = row[0];
        for (int c = 1; c < C; ++c) {
            const float v = row[c];
            if (pn2_beats(v, best)) { best = v; arg = c; }
        }
    }
    return arg;
}
