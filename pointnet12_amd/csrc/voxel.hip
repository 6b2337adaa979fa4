// Voxel-grid downsampling on the device: one row per occupied cell of a regular grid, for a batch of clouds that lie back to back
// in HBM -- the grid subsample of every LiDAR code base (open3d's voxel_down_sample picks the cells the same way), with the kept
// COUNT left in device memory, a STABLE compaction and an exact inverse map from every input row to the row that stands for it.
//
//   pn2_voxel_grid   at most six plain launches on the caller's stream, no thread ever waits for another thread's write:
//     voxel_clear_kernel    every slot of every cloud's hash table to (key = EMPTY, lowest row = INT_MAX, population = 0): the
//                           workspace arrives holding garbage;
//     voxel_insert_kernel   one thread per row: the cell key of include/pn2.h in fp64, an open-addressing insert (64-bit atomicCAS
//                           on the key word; a slot that holds another key simply moves on; the probe loop is bounded by the
//                           capacity), then atomicMin of the row number and atomicAdd of the population on that slot; the row's slot
//                           is remembered in the workspace, so no later pass probes again;
//     voxel_flag_kernel     a LATER launch (the launch boundary orders it behind every insert): row i stands for its voxel iff the
//                           slot's lowest row is i; a one-byte flag per row and the tile's count (__ballot + popcount);
//     voxel_offsets_kernel  one wave per cloud: exclusive prefix sum of its tiles' counts, the cloud's voxel count, the "row_count
//                           above max_rows" bit;
//     voxel_write_kernel    rank inside the wave from the ballot, the sixteen 64-row segments of a tile ordered through LDS; every
//                           representative copies its row, label, row number and its slot's population, and leaves its RANK in
//                           the slot (the lowest-row word is no longer needed);
//     voxel_inverse_kernel  every row reads the rank from its slot (skipped without an `inverse`).
//   Which slot a key lands in depends on who wins a CAS; nothing that is written out does: the representative is an integer
//   minimum, the population an integer sum, the order a prefix sum over row numbers.  The result is the same from run to run.
//
// This file is built with -ffp-contract=off: q = floor(((double)p - origin) / voxel) is two separately rounded fp64 operations.
#include <cmath>
#include "pn2_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / PN2_WAVE;
constexpr int kRounds = PN2_VOXEL_TILE / kThreads;                  // rows per thread of the compaction passes
constexpr int kSegments = kRounds * kWaves;                         // 64-row segments of a tile, in row order
static_assert(PN2_VOXEL_TILE % kThreads == 0 && kThreads % PN2_WAVE == 0, "a tile is a whole number of workgroup rounds");
constexpr unsigned long long kEmpty = ~0ull;                        // no key: a key has 63 bits
constexpr int kNoRow = 0x7FFFFFFF;
constexpr int kClearBlocks = 1 << 16;

struct alignas(16) Slot {
    unsigned long long key;
    int low;                                                        // the lowest row of the voxel; after voxel_write_kernel: its rank
    int pop;                                                        // valid rows in the voxel
};
static_assert(sizeof(Slot) == 16, "one slot is one 16-byte word");

struct Grid {
    double origin[3], voxel[3];
};

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

__device__ __forceinline__ int clamped_rows(const int64_t *row_count, int b, int max_rows) {
    const int64_t n = row_count[b];
    return n < 0 ? 0 : (n > max_rows ? max_rows : (int)n);
}

__global__ __launch_bounds__(kThreads) void voxel_clear_kernel(uint4 *__restrict__ table, int64_t slots) {
    const uint4 empty = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, (unsigned)kNoRow, 0u);
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < slots; i += (int64_t)gridDim.x * kThreads) table[i] = empty;
}

// the cell of one coordinate, biased to [0, 2^21); false: outside the grid (or not finite)
__device__ __forceinline__ bool cell_of(float p, double origin, double voxel, unsigned long long &biased) {
    const double q = floor(((double)p - origin) / voxel);
    if (!(q >= -1048576.0 && q < 1048576.0)) return false;
    biased = (unsigned long long)((long long)q + 1048576ll);
    return true;
}

__device__ __forceinline__ unsigned mix(unsigned long long k) {    // (murmur3's finaliser; the choice shows in no output)
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (unsigned)k;
}

template <bool kVec4>
__global__ __launch_bounds__(kThreads) void voxel_insert_kernel(const float *__restrict__ pts, int ld,
                                                                const int64_t *__restrict__ row_begin,
                                                                const int64_t *__restrict__ row_count, int max_rows, Grid grid,
                                                                Slot *__restrict__ table, unsigned cap, int *__restrict__ row_slot,
                                                                int64_t rows_pad, int *__restrict__ err) {
    const int b = blockIdx.y;
    const int n = clamped_rows(row_count, b, max_rows);
    const int64_t i64 = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if ((int64_t)blockIdx.x * kThreads >= n) return;                // (uniform over the workgroup)
    const bool live = i64 < n;
    const int i = (int)i64;
    int slot = -1;
    bool dropped = false;
    if (live) {
        const int64_t row = row_begin[b] + i;
        float x, y, z;
        if (kVec4) {
            const float4 p = reinterpret_cast<const float4 *>(pts)[row];
            x = p.x, y = p.y, z = p.z;
        } else {
            const float *p = pts + row * ld;
            x = p[0], y = p[1], z = p[2];
        }
        unsigned long long cx, cy, cz;
        if (cell_of(x, grid.origin[0], grid.voxel[0], cx) && cell_of(y, grid.origin[1], grid.voxel[1], cy) &&
            cell_of(z, grid.origin[2], grid.voxel[2], cz)) {
            const unsigned long long key = (cx << 42) | (cy << 21) | cz;
            Slot *tab = table + (int64_t)b * cap;
            unsigned s = mix(key) & (cap - 1);
            for (unsigned probe = 0; probe < cap; ++probe) {        // bounded: at most one pass over the table
                const unsigned long long seen = atomicCAS(&tab[s].key, kEmpty, key);
                if (seen == kEmpty || seen == key) {
                    slot = (int)s;
                    break;
                }
                s = (s + 1) & (cap - 1);                            // another voxel's slot: move on, never wait
            }
            if (slot >= 0) {
                atomicMin(&tab[slot].low, i);
                atomicAdd(&tab[slot].pop, 1);
            }
            // (slot < 0 cannot happen: the table has at least twice as many slots as the cloud has rows)
        } else {
            dropped = true;
        }
        row_slot[(int64_t)b * rows_pad + i] = slot;
    }
    if (err != nullptr && __any(dropped) && (threadIdx.x & (PN2_WAVE - 1)) == 0) atomicOr(err, PN2_VOXEL_ERR_RANGE);
}

__global__ __launch_bounds__(kThreads) void voxel_flag_kernel(const int64_t *__restrict__ row_count, int max_rows,
                                                              const Slot *__restrict__ table, unsigned cap,
                                                              const int *__restrict__ row_slot, unsigned char *__restrict__ flags,
                                                              int *__restrict__ tile_count, int tiles) {
    __shared__ int s_count[kWaves];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int n = clamped_rows(row_count, b, max_rows);
    const int64_t t0 = (int64_t)tile * PN2_VOXEL_TILE;
    if (t0 >= n) return;
    const int left = (int)(n - t0 < PN2_VOXEL_TILE ? n - t0 : PN2_VOXEL_TILE);
    const int64_t at = ((int64_t)b * tiles + tile) * PN2_VOXEL_TILE;
    const Slot *tab = table + (int64_t)b * cap;
    int kept = 0;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const int i = r * kThreads + (int)threadIdx.x;
        bool keep = false;
        if (i < left) {
            const int s = row_slot[at + i];
            keep = s >= 0 && tab[s].low == (int)(t0 + i);
        }
        flags[at + i] = keep ? 1 : 0;                               // every row of the tile, the ones beyond the cloud as 0
        kept += __popcll(__ballot(keep));
    }
    const int lane = threadIdx.x & (PN2_WAVE - 1), wave = threadIdx.x / PN2_WAVE;
    if (lane == 0) s_count[wave] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) total += s_count[w];
        tile_count[(int64_t)b * tiles + tile] = total;
    }
}

__global__ __launch_bounds__(PN2_WAVE) void voxel_offsets_kernel(const int64_t *__restrict__ row_count, int max_rows,
                                                                 const int *__restrict__ tile_count, int *__restrict__ tile_offset,
                                                                 int tiles, int64_t *__restrict__ out_count, int *__restrict__ err) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = clamped_rows(row_count, b, max_rows);
    const int active = (int)(((int64_t)n + PN2_VOXEL_TILE - 1) / PN2_VOXEL_TILE);     // <= tiles: n <= max_rows
    const int *cnt = tile_count + (int64_t)b * tiles;
    int *off = tile_offset + (int64_t)b * tiles;
    int carry = 0;
    for (int first = 0; first < active; first += PN2_WAVE) {
        const int i = first + lane;
        const int v = i < active ? cnt[i] : 0;
        int incl = v;
#pragma unroll
        for (int d = 1; d < PN2_WAVE; d <<= 1) {
            const int up = __shfl_up(incl, d, PN2_WAVE);
            if (lane >= d) incl += up;
        }
        if (i < active) off[i] = carry + incl - v;
        carry += __shfl(incl, PN2_WAVE - 1, PN2_WAVE);
    }
    if (lane == 0) {
        out_count[b] = carry;
        if (err != nullptr && row_count[b] > max_rows) atomicOr(err, PN2_VOXEL_ERR_ROWS);
    }
}

template <bool kVec4>
__global__ __launch_bounds__(kThreads) void voxel_write_kernel(const float *__restrict__ pts, int ld, const int32_t *__restrict__ labels_in,
                                                               const int64_t *__restrict__ row_begin,
                                                               const int64_t *__restrict__ row_count, int max_rows,
                                                               Slot *__restrict__ table, unsigned cap, const int *__restrict__ row_slot,
                                                               const unsigned char *__restrict__ flags,
                                                               const int *__restrict__ tile_offset, int tiles,
                                                               const int64_t *__restrict__ out_begin, float *__restrict__ out_points,
                                                               int32_t *__restrict__ out_labels, int32_t *__restrict__ out_index,
                                                               int32_t *__restrict__ n_points, int leave_rank) {
    __shared__ int s_seg[kSegments];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int n = clamped_rows(row_count, b, max_rows);
    const int64_t t0 = (int64_t)tile * PN2_VOXEL_TILE;
    if (t0 >= n) return;
    const int64_t base = row_begin[b] + t0;
    const int64_t at = ((int64_t)b * tiles + tile) * PN2_VOXEL_TILE;
    const int lane = threadIdx.x & (PN2_WAVE - 1), wave = threadIdx.x / PN2_WAVE;
    bool keep[kRounds];
    int rank[kRounds];
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        keep[r] = flags[at + r * kThreads + (int)threadIdx.x] != 0;
        const unsigned long long m = __ballot(keep[r]);
        rank[r] = __popcll(m & ((1ull << lane) - 1ull));            // representatives of this segment before this lane
        if (lane == 0) s_seg[r * kWaves + wave] = __popcll(m);
    }
    __syncthreads();
    const int first = tile_offset[(int64_t)b * tiles + tile];       // the rank, inside the cloud, of the tile's first representative
    const int64_t out0 = out_begin[b];
    Slot *tab = table + (int64_t)b * cap;
    int before = 0, seg = 0;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const int mine = r * kWaves + wave;
        for (; seg < mine; ++seg) before += s_seg[seg];
        if (keep[r]) {
            const int i = r * kThreads + (int)threadIdx.x;
            const int rk = first + before + rank[r];
            const int64_t o = out0 + rk;
            const int s = row_slot[at + i];
            if (out_points != nullptr) {
                if (kVec4) {
                    reinterpret_cast<float4 *>(out_points)[o] = reinterpret_cast<const float4 *>(pts)[base + i];
                } else {
                    const uint32_t *src = reinterpret_cast<const uint32_t *>(pts) + (base + i) * ld;
                    uint32_t *dst = reinterpret_cast<uint32_t *>(out_points) + o * ld;
                    for (int c = 0; c < ld; ++c) dst[c] = src[c];   // dword moves: the row bit for bit
                }
            }
            if (out_labels != nullptr) out_labels[o] = labels_in != nullptr ? labels_in[base + i] : 0;
            if (out_index != nullptr) out_index[o] = (int32_t)(t0 + i);
            if (n_points != nullptr) n_points[o] = tab[s].pop;
            if (leave_rank) tab[s].low = rk;                        // (nothing in this launch reads the word)
        }
    }
}

__global__ __launch_bounds__(kThreads) void voxel_inverse_kernel(const int64_t *__restrict__ row_begin,
                                                                 const int64_t *__restrict__ row_count, int max_rows,
                                                                 const Slot *__restrict__ table, unsigned cap,
                                                                 const int *__restrict__ row_slot, int64_t rows_pad,
                                                                 int32_t *__restrict__ inverse) {
    const int b = blockIdx.y;
    const int n = clamped_rows(row_count, b, max_rows);
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int s = row_slot[(int64_t)b * rows_pad + i];
    inverse[row_begin[b] + i] = s >= 0 ? table[(int64_t)b * cap + s].low : -1;
}

inline int voxel_tiles(int64_t max_rows) { return max_rows == 0 ? 1 : (int)pn2_cdiv(max_rows, PN2_VOXEL_TILE); }
inline int64_t voxel_capacity(int64_t max_rows) {                  // a power of two >= 2 * max_rows (and >= 64)
    int64_t cap = 64;
    while (cap < 2 * max_rows) cap <<= 1;
    return cap;
}
inline int64_t round16(int64_t v) { return (v + 15) / 16 * 16; }
inline bool shape_ok(int B, int64_t max_rows) { return B >= 1 && B <= 65535 && max_rows >= 0 && max_rows <= PN2_VOXEL_MAX_ROWS; }

}  // namespace

extern "C" {

int64_t pn2_voxel_grid_workspace_bytes(int B, int64_t max_rows) {
    if (!shape_ok(B, max_rows)) return PN2_EINVAL;
    const int64_t rows = (int64_t)B * voxel_tiles(max_rows) * PN2_VOXEL_TILE;
    // the tables, a slot number per row, a flag per row, a count and an offset per tile
    return (int64_t)B * voxel_capacity(max_rows) * (int64_t)sizeof(Slot) + rows * (int64_t)sizeof(int) + rows +
           2 * round16((int64_t)B * voxel_tiles(max_rows) * (int64_t)sizeof(int));
}

int pn2_voxel_grid(const float *pts, int ld, const int32_t *labels_in, const int64_t *row_begin, const int64_t *row_count, int B,
                   int64_t max_rows, const double *origin, const double *voxel, const int64_t *out_begin, float *out_points,
                   int32_t *out_labels, int32_t *out_index, int64_t *out_count, int32_t *inverse, int32_t *n_points, int *err,
                   void *workspace, pn2_stream_t stream) {
    PN2_CHECK_ARG(pts && row_begin && row_count && origin && voxel && out_begin && out_count && workspace);
    PN2_CHECK_ARG(shape_ok(B, max_rows) && ld >= 3 && ld <= 16);
    PN2_CHECK_ARG(aligned4(pts) && aligned4(out_points) && aligned16(workspace));
    Grid grid;
    for (int a = 0; a < 3; ++a) {
        PN2_CHECK_ARG(std::isfinite(origin[a]) && std::isfinite(voxel[a]) && voxel[a] > 0.0);
        grid.origin[a] = origin[a];
        grid.voxel[a] = voxel[a];
    }
    const int tiles = voxel_tiles(max_rows);
    const int64_t cap = voxel_capacity(max_rows), rows_pad = (int64_t)tiles * PN2_VOXEL_TILE, slots = (int64_t)B * cap;
    unsigned char *at = static_cast<unsigned char *>(workspace);
    Slot *table = reinterpret_cast<Slot *>(at);
    at += slots * (int64_t)sizeof(Slot);
    int *row_slot = reinterpret_cast<int *>(at);
    at += (int64_t)B * rows_pad * (int64_t)sizeof(int);
    unsigned char *flags = at;
    at += (int64_t)B * rows_pad;
    int *tile_count = reinterpret_cast<int *>(at);
    at += round16((int64_t)B * tiles * (int64_t)sizeof(int));
    int *tile_offset = reinterpret_cast<int *>(at);
    const bool vec4 = ld == 4 && aligned16(pts) && (out_points == nullptr || aligned16(out_points));
    const hipStream_t s = pn2_s(stream);
    const dim3 by_tile((unsigned)tiles, (unsigned)B), by_row((unsigned)(rows_pad / kThreads), (unsigned)B);
    const int64_t clear_blocks = pn2_cdiv(slots, kThreads);
    hipLaunchKernelGGL(voxel_clear_kernel, dim3((unsigned)(clear_blocks < kClearBlocks ? clear_blocks : kClearBlocks)), dim3(kThreads),
                       0, s, reinterpret_cast<uint4 *>(table), slots);
    if (vec4)
        hipLaunchKernelGGL(voxel_insert_kernel<true>, by_row, dim3(kThreads), 0, s, pts, ld, row_begin, row_count, (int)max_rows, grid,
                           table, (unsigned)cap, row_slot, rows_pad, err);
    else
        hipLaunchKernelGGL(voxel_insert_kernel<false>, by_row, dim3(kThreads), 0, s, pts, ld, row_begin, row_count, (int)max_rows, grid,
                           table, (unsigned)cap, row_slot, rows_pad, err);
    hipLaunchKernelGGL(voxel_flag_kernel, by_tile, dim3(kThreads), 0, s, row_count, (int)max_rows, table, (unsigned)cap, row_slot, flags,
                       tile_count, tiles);
    hipLaunchKernelGGL(voxel_offsets_kernel, dim3((unsigned)B), dim3(PN2_WAVE), 0, s, row_count, (int)max_rows, tile_count, tile_offset,
                       tiles, out_count, err);
    const int leave_rank = inverse != nullptr;
    if (out_points || out_labels || out_index || n_points || leave_rank) {
        if (vec4)
            hipLaunchKernelGGL(voxel_write_kernel<true>, by_tile, dim3(kThreads), 0, s, pts, ld, labels_in, row_begin, row_count,
                               (int)max_rows, table, (unsigned)cap, row_slot, flags, tile_offset, tiles, out_begin, out_points, out_labels,
                               out_index, n_points, leave_rank);
        else
            hipLaunchKernelGGL(voxel_write_kernel<false>, by_tile, dim3(kThreads), 0, s, pts, ld, labels_in, row_begin, row_count,
                               (int)max_rows, table, (unsigned)cap, row_slot, flags, tile_offset, tiles, out_begin, out_points, out_labels,
                               out_index, n_points, leave_rank);
    }
    if (leave_rank)
        hipLaunchKernelGGL(voxel_inverse_kernel, by_row, dim3(kThreads), 0, s, row_begin, row_count, (int)max_rows, table, (unsigned)cap,
                           row_slot, rows_pad, inverse);
    return pn2_launch_status();
}

}  // extern "C"
