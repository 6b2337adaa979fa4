// The tiled fp64 sum of the refit kernels (icp.hip: 29 words, plane.hip: 10, corr_ransac.hip: 17), in ONE place.  A cloud's rows are
// cut into tiles of kSumTile; an accumulate kernel runs one workgroup of kSumThreads per tile, a finish kernel one per cloud.
//
//   rows     lane t of tile `tile` takes the rows pn2_tile_row(tile, r), r = 0 .. kSumRows - 1, one after another, and adds each
//            row's terms to its W accumulators in registers.
//   partial  pn2_tile_partial: per word a butterfly over the wave (pn2_wave_sum_f64), lane 0 of each wave to LDS, ONE barrier,
//            thread t < W adds the waves in wave order starting from wave 0's value, one partial of W doubles per tile.
//   total    pn2_tile_total: thread (k, c) = (t & 31, t >> 5) adds word k of the tiles c, c + kSumChunks, ... in ascending order
//            starting from 0.0, ONE barrier, thread 0 adds the chunks in chunk order starting from chunk 0's value.
//
// The order of every sum is a function of (B, N) alone -- which lane holds which row, the butterfly, the wave order, the chunk
// assignment -- and of nothing the hardware decides: the bytes are the same from run to run.  No float atomics, no thread waits for
// another thread's write.  The callers are built with -ffp-contract=off and keep what is theirs: the early return of a cloud that
// takes no part (uniform over the workgroup, BEFORE either function's barrier) and "a tile at or beyond the count adds nothing and
// writes zeros" (the workspace arrives holding anything).
#pragma once
#include "pn2_common.h"

constexpr int kSumThreads = 256;                                    // workgroup of both kernels
constexpr int kSumWaves = kSumThreads / PN2_WAVE;
constexpr int kSumRows = 4;                                         // rows per lane
constexpr int kSumTile = kSumThreads * kSumRows;                    // rows per workgroup
constexpr int kSumChunks = 8;                                       // of the finish kernel
static_assert(kSumChunks * 32 == kSumThreads, "the finish kernel is kSumChunks chunks of 32 words");

// row of trip r of this lane in tile `tile`
__device__ __forceinline__ int64_t pn2_tile_row(int tile, int r) { return (int64_t)tile * kSumTile + (int64_t)r * kSumThreads + threadIdx.x; }

// The whole workgroup calls it once: acc, this lane's W sums; s_wave, the caller's LDS; out, the W doubles of this tile's partial.
template <int W>
__device__ __forceinline__ void pn2_tile_partial(const double (&acc)[W], double (&s_wave)[kSumWaves][W], double *__restrict__ out) {
    static_assert(W <= 32, "pn2_tile_total gives a word to each of 32 threads");
    const int t = threadIdx.x, lane = t & (PN2_WAVE - 1), wave = t >> 6;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const double v = pn2_wave_sum_f64(acc[k]);
        if (lane == 0) s_wave[wave][k] = v;
    }
    __syncthreads();
    if (t < W) {
        double v = s_wave[0][t];
        for (int k = 1; k < kSumWaves; ++k) v = v + s_wave[k][t];
        out[t] = v;
    }
}

// The whole workgroup calls it once: partial, the cloud's `tiles` partials of W doubles; s_chunk, the caller's LDS.  True on thread
// 0 alone, which then holds the W totals in S: the caller's scalar tail follows an `if (!pn2_tile_total(...)) return;`.
template <int W>
__device__ __forceinline__ bool pn2_tile_total(const double *__restrict__ partial, int tiles, double (&s_chunk)[kSumChunks][32], double (&S)[W]) {
    static_assert(W <= 32, "a word to each of 32 threads");
    const int t = threadIdx.x, k = t & 31, c = t >> 5;
    double v = 0.0;
    if (k < W)
        for (int tile = c; tile < tiles; tile += kSumChunks) v = v + partial[(int64_t)tile * W + k];
    s_chunk[c][k] = v;
    __syncthreads();
    if (t != 0) return false;
#pragma unroll
    for (int q = 0; q < W; ++q) {
        double s = s_chunk[0][q];
#pragma unroll
        for (int h = 1; h < kSumChunks; ++h) s = s + s_chunk[h][q];
        S[q] = s;
    }
    return true;
}
