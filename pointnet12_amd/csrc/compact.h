// The stable tile compaction of scan.hip (pn2_scan_filter) and voxel.hip (pn2_voxel_grid), in ONE place: kept rows keep their order
// and their positions come from prefix sums alone -- no atomics, no workgroup ever waits on another, the output is byte-identical
// from run to run.  Three launches, a launch boundary is the only ordering between them:
//   a flag kernel     one workgroup per tile of kCompactTile rows, built on pn2_compact_flag_tile: a one-byte flag per row and the
//                     tile's kept count (__ballot + popcount per wave, the four waves summed through LDS);
//   pn2_compact_offsets_kernel   one wave per cloud: exclusive prefix sum of its tiles' counts (pn2_wave_row_excl_scan), the
//                     cloud's kept count, the caller's "row_count above max_rows" bit;
//   a write kernel    one workgroup per tile, built on pn2_compact_write_tile: rank inside the wave from the ballot, the sixteen
//                     64-row segments of the tile ordered through LDS; the caller's lambda stores every kept row at its rank.
// The caller's kernels compute b, tile, n = pn2_clamped_rows(...), t0 = tile * kCompactTile and return when t0 >= n (uniform over
// the workgroup: both helpers hold a barrier), so a captured launch sized by max_rows stays valid when the device-side count changes.
#pragma once
#include "pn2_common.h"
#include "wave_ops.h"

constexpr int kCompactTile = 1024;                                  // rows per workgroup of the flag and the write pass
static_assert(PN2_SCAN_TILE == kCompactTile && PN2_VOXEL_TILE == kCompactTile, "both entry points share this code and its tile");
constexpr int kCompactThreads = 256;
constexpr int kCompactWaves = kCompactThreads / PN2_WAVE;
constexpr int kCompactRounds = kCompactTile / kCompactThreads;      // rows per thread; row = round * kCompactThreads + thread
constexpr int kCompactSegments = kCompactRounds * kCompactWaves;    // 64-row segments of a tile, in row order
static_assert(kCompactTile % kCompactThreads == 0 && kCompactThreads % PN2_WAVE == 0, "a tile is a whole number of workgroup rounds");

// The compaction's part of a workspace: a flag per row of every tile, a count and an offset per tile (each 16-byte aligned when
// the base is), taken from the caller's arena.
struct Pn2Compact {
    unsigned char *flags;
    int *tile_count, *tile_offset;
    int tiles;                                                      // per cloud
};
static inline int pn2_compact_tiles(int64_t max_rows) { return max_rows == 0 ? 1 : (int)pn2_cdiv(max_rows, kCompactTile); }
static inline Pn2Compact pn2_compact_take(Pn2Arena &a, int B, int64_t max_rows) {
    const int tiles = pn2_compact_tiles(max_rows);
    const int64_t n = (int64_t)B * tiles;
    return {a.take<unsigned char>(n * kCompactTile), a.take<int>(n), a.take<int>(n), tiles};
}

// How many of a tile's kCompactTile rows satisfy pred(i), i = round * kCompactThreads + thread: a ballot and a popcount per wave and
// round, the wave totals summed through LDS, one store of the count.  Holds one barrier.
template <class Pred>
__device__ __forceinline__ void pn2_compact_count_tile(int *__restrict__ tile_count, Pred pred) {
    __shared__ int s_count[kCompactWaves];
    int n = 0;
#pragma unroll
    for (int r = 0; r < kCompactRounds; ++r) n += __popcll(__ballot(pred(r * kCompactThreads + (int)threadIdx.x)));
    if ((threadIdx.x & (PN2_WAVE - 1)) == 0) s_count[threadIdx.x / PN2_WAVE] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < kCompactWaves; ++w) total += s_count[w];
        *tile_count = total;
    }
}

// The flag pass of one tile with `left` rows (1 .. kCompactTile) inside the cloud: keep_row(i) is evaluated for i < left only;
// every row of the tile gets its flag, the ones beyond the cloud 0; one store of the tile's count.
template <class Keep>
__device__ __forceinline__ void pn2_compact_flag_tile(int left, unsigned char *__restrict__ flags_of_tile, int *__restrict__ tile_count,
                                                      Keep keep_row) {
    pn2_compact_count_tile(tile_count, [&](int i) {
        const bool keep = i < left && keep_row(i);
        flags_of_tile[i] = keep ? 1 : 0;
        return keep;
    });
}

// rank[r] = the flagged rows of the tile before this thread's row of round r (itself not counted): inside its 64-row segment from
// the ballot, the sixteen segments of the tile ordered through LDS.  Holds one barrier.
__device__ __forceinline__ void pn2_compact_rank_tile(const bool (&flag)[kCompactRounds], int (&rank)[kCompactRounds]) {
    __shared__ int s_seg[kCompactSegments];
    const int lane = threadIdx.x & (PN2_WAVE - 1), wave = threadIdx.x / PN2_WAVE;
#pragma unroll
    for (int r = 0; r < kCompactRounds; ++r) {
        const unsigned long long m = __ballot(flag[r]);
        rank[r] = __popcll(m & ((1ull << lane) - 1ull));            // flagged rows of this segment before this lane
        if (lane == 0) s_seg[r * kCompactWaves + wave] = __popcll(m);
    }
    __syncthreads();
    int before = 0, seg = 0;                                        // flagged rows of the tile in the segments before segment `seg`
#pragma unroll
    for (int r = 0; r < kCompactRounds; ++r) {
        const int mine = r * kCompactWaves + wave;
        for (; seg < mine; ++seg) before += s_seg[seg];
        rank[r] += before;
    }
}

// The write pass of one tile: emit(i, rank) for every kept row i of the tile, rank = kept rows of the tile before it.
template <class Emit>
__device__ __forceinline__ void pn2_compact_write_tile(const unsigned char *__restrict__ flags_of_tile, Emit emit) {
    bool keep[kCompactRounds];
    int rank[kCompactRounds];
#pragma unroll
    for (int r = 0; r < kCompactRounds; ++r) keep[r] = flags_of_tile[r * kCompactThreads + (int)threadIdx.x] != 0;
    pn2_compact_rank_tile(keep, rank);
#pragma unroll
    for (int r = 0; r < kCompactRounds; ++r)
        if (keep[r]) emit(r * kCompactThreads + (int)threadIdx.x, rank[r]);
}

namespace {

__global__ __launch_bounds__(PN2_WAVE) void pn2_compact_offsets_kernel(const int64_t *__restrict__ row_count, int max_rows,
                                                                       const int *__restrict__ tile_count,
                                                                       int *__restrict__ tile_offset, int tiles,
                                                                       int64_t *__restrict__ out_count, int *__restrict__ err,
                                                                       int rows_bit) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = pn2_clamped_rows(row_count, b, max_rows);
    const int active = (int)(((int64_t)n + kCompactTile - 1) / kCompactTile);          // <= tiles: n <= max_rows
    const int kept = pn2_wave_row_excl_scan(tile_count + (int64_t)b * tiles, tile_offset + (int64_t)b * tiles, active);    // at most n < 2^31
    if (lane == 0) {
        out_count[b] = kept;
        if (err != nullptr && row_count[b] > max_rows) atomicOr(err, rows_bit);
    }
}

}  // namespace
