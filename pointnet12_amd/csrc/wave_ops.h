// The wave and workgroup building blocks of the integer kernels (compaction, counting sorts, radix sort, slot-table counters), in
// ONE place.  Every function is called by WHOLE waves of a one-dimensional workgroup (lane = threadIdx.x & 63); all of them are
// integer: what they return is the same whatever the order the hardware takes.
#pragma once
#include "pn2_common.h"

// inclusive prefix sum of one int per lane over the wave
__device__ __forceinline__ int pn2_wave_incl_scan(int v) {
    const int t = threadIdx.x, lane = t & (PN2_WAVE - 1);
#pragma unroll
    for (int d = 1; d < PN2_WAVE; d <<= 1) {
        const int up = __shfl_up(v, d, PN2_WAVE);
        if (lane >= d) v += up;
    }
    return v;
}

// Exclusive prefix sum of one int per thread over the workgroup, in thread order: the wave scans by shuffle, the wave totals through
// `s_wave`, the caller's LDS array of one int per wave.  It holds ONE barrier, between the store of the wave totals and their loads:
// every thread of the workgroup calls it, and a caller that calls it again on the same array puts a barrier of its own in between.
// A wave adds the totals of the waves below it and no more, so the function needs no wave count: workgroups of 4 and of 16 waves use it.
__device__ __forceinline__ int pn2_block_excl_scan(int v, int *s_wave) {
    const int t = threadIdx.x, lane = t & (PN2_WAVE - 1), wave = t >> 6;
    const int incl = pn2_wave_incl_scan(v);
    if (lane == PN2_WAVE - 1) s_wave[wave] = incl;
    __syncthreads();
    int before = incl - v;
    for (int w = 0; w < wave; ++w) before += s_wave[w];
    return before;
}

// One wave, a row of n counts: out[i] = in[0] + ... + in[i - 1] (in place when out == in), 64 counts a step with a carry between.
// Returns the row's sum on every lane.
__device__ __forceinline__ int pn2_wave_row_excl_scan(const int *in, int *out, int n) {
    const int lane = threadIdx.x & (PN2_WAVE - 1);
    int carry = 0;
    for (int first = 0; first < n; first += PN2_WAVE) {
        const int i = first + lane;
        const int v = i < n ? in[i] : 0;
        const int incl = pn2_wave_incl_scan(v);
        if (i < n) out[i] = carry + incl - v;
        carry += __shfl(incl, PN2_WAVE - 1, PN2_WAVE);
    }
    return carry;
}

__device__ __forceinline__ unsigned long long pn2_wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, PN2_WAVE);
    return v;
}

// Same-key combine in front of an atomic: neighbouring rows mostly hold one key, so instead of 64 same-address atomics the lowest
// waiting lane leads a round, the lanes that hold its key vote, and ONE lane acts for all of them.  Up to ROUNDS keys per call;
// round(voter, leader, votes) is called by the whole wave: is this lane a voter of the round, the leader's lane number, the mask of
// the voters (the leader is one of them).  Returns whether the lane is still waiting: the caller sends those lanes alone, with
// whatever its single-lane form is.
template <int ROUNDS, class Key, class Round>
__device__ __forceinline__ bool pn2_wave_combine(Key key, bool live, Round round) {
#pragma nounroll                                                    // (one copy of the caller's round: the later rounds serve few lanes)
    for (int r = 0; r < ROUNDS; ++r) {
        const unsigned long long waiting = __ballot(live);
        if (waiting == 0ull) break;                                 // (uniform over the wave)
        const int leader = __ffsll((long long)waiting) - 1;
        const Key its = __shfl(key, leader, PN2_WAVE);
        const bool same = live && key == its;
        round(same, leader, __ballot(same));
        live = live && !same;
    }
    return live;
}
