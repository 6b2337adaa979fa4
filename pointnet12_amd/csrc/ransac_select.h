// The select step of the RANSAC entry points (plane.hip, corr_ransac.hip), in ONE place: the scoring pass left one int32 per (tile of
// kScoreTile rows, hypothesis); one workgroup per cloud adds them per hypothesis and keeps the largest count, the lowest h among equals.
// Integers throughout: the result does not depend on the order the hardware takes.
#pragma once
#include "pn2_common.h"

constexpr int kScoreTile = 512;                                     // rows per scoring workgroup

// (count + 1) in the high word, ~h in the low one: the largest count, the lowest h among equals; 0 = no valid hypothesis
__device__ __forceinline__ unsigned long long ransac_key(int64_t count, int h) {
    return ((unsigned long long)(count + 1) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)h);
}

struct RansacBest {
    bool any;                                                       // a valid hypothesis exists
    int h;                                                          // the best one, -1 without any
    int64_t count;                                                  // its inliers, 0 without any
};

// The whole workgroup (WAVES waves) calls it once for cloud b of n rows: thread t adds the tile counts of hypotheses t, t + 64 WAVES,
// ... in tile order over the tiles the scoring pass wrote, writes hyp_count (if asked for; -1 for an invalid hypothesis) and keeps
// its best key; the keys meet through a wave maximum and `s_key`, the caller's LDS (ONE barrier).  A hypothesis is `stride` doubles
// in hyp and valid when its word 0 is not NaN.  True on thread 0 alone, which then holds the result in `best`.
template <int WAVES>
__device__ __forceinline__ bool ransac_select(int b, int n, int H, const double *__restrict__ hyp, int stride, int tiles,
                                              const int32_t *__restrict__ tile_count, int32_t *__restrict__ hyp_count,
                                              unsigned long long (&s_key)[WAVES], RansacBest &best) {
    const int t = threadIdx.x;
    const int live = (int)(((int64_t)n + kScoreTile - 1) / kScoreTile);
    unsigned long long key = 0;
    for (int h = t; h < H; h += WAVES * PN2_WAVE) {
        const double w0 = hyp[((int64_t)b * H + h) * stride];
        const bool valid = w0 == w0;
        int64_t c = 0;
        for (int tile = 0; tile < live; ++tile) c += tile_count[((int64_t)b * tiles + tile) * H + h];
        if (hyp_count != nullptr) hyp_count[(int64_t)b * H + h] = valid ? (int32_t)c : -1;
        const unsigned long long k = ransac_key(c, h);
        if (valid && k > key) key = k;
    }
    key = pn2_wave_max_u64(key);
    if ((t & (PN2_WAVE - 1)) == 0) s_key[t >> 6] = key;
    __syncthreads();
    if (t != 0) return false;
    for (int k = 1; k < WAVES; ++k) key = s_key[k] > key ? s_key[k] : key;
    best.any = key != 0;
    best.h = best.any ? (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)) : -1;
    best.count = best.any ? (int64_t)(key >> 32) - 1 : 0;
    return true;
}
