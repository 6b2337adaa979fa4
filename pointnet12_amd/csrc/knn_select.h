// The register-resident K-best selection of knn.hip's kernel, with a LEXICOGRAPHIC compare on the (d2, index) pair: grid_knn.hip
// meets its candidates cell by cell, in an order that differs from run to run, so the index has to take part in the compare for
// the outcome not to depend on that order (knn.hip meets them in ascending index and gets by with a strict < on d2 alone).
#pragma once
#include "pn2_common.h"

// (d, j) before (bd, bi) in ascending (d2, index) order; a NaN d is before nothing
__device__ __forceinline__ bool pn2_pair_before(float d, int j, float bd, int bi) { return d < bd || (d == bd && j < bi); }

// A lane's CAP best pairs, ascending, in registers: (d, j) is tested against the worst of them first and only then walks the
// compare-and-shift chain -- fully unrolled over the compile-time capacity, so every array index is a constant and nothing goes
// to scratch.  Empty slots hold (+inf, M) with M above every index: they sort behind every candidate.
template <int CAP>
__device__ __forceinline__ void pn2_select_insert(float (&bd)[CAP], int (&bi)[CAP], float d, int j) {
    if (!pn2_pair_before(d, j, bd[CAP - 1], bi[CAP - 1])) return;
    bool lt[CAP];
#pragma unroll
    for (int s = 0; s < CAP; ++s) lt[s] = pn2_pair_before(d, j, bd[s], bi[s]);
#pragma unroll
    for (int s = CAP - 1; s > 0; --s) {                             // slot s: the old slot s-1 moves down, or the pair lands here, or it stays
        bd[s] = lt[s - 1] ? bd[s - 1] : (lt[s] ? d : bd[s]);
        bi[s] = lt[s - 1] ? bi[s - 1] : (lt[s] ? j : bi[s]);
    }
    bd[0] = lt[0] ? d : bd[0];
    bi[0] = lt[0] ? j : bi[0];
}
