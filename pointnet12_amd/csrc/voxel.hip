// Voxel-grid downsampling on the device: one row per occupied cell of a regular grid, for a batch of clouds that lie back to back
// in HBM -- the grid subsample of every LiDAR code base (open3d's voxel_down_sample picks the cells the same way), with the kept
// COUNT left in device memory, a STABLE compaction and an exact inverse map from every input row to the row that stands for it.
//
//   pn2_voxel_grid   at most six plain launches on the caller's stream, no thread ever waits for another thread's write: the
//   open-addressing table of slot_table.h, then the stable tile compaction of compact.h over "row i stands for its voxel":
//     pn2_slot_clear_kernel every slot of every cloud's table to (key = EMPTY, lowest row = INT_MAX, population = 0);
//     voxel_insert_kernel   one thread per row: the cell key of include/pn2.h in fp64 (voxel_cell.h), pn2_slot_claim, then atomicMin of the row
//                           number and atomicAdd of the population on that slot; the row's slot is remembered in the workspace,
//                           so no later pass probes again;
//     voxel_flag_kernel     a LATER launch (the launch boundary orders it behind every insert): row i stands for its voxel iff the
//                           slot's lowest row is i;
//     pn2_compact_offsets_kernel   the cloud's voxel count, the "row_count above max_rows" bit;
//     voxel_write_kernel    every representative copies its row, label, row number and its slot's population, and leaves its RANK
//                           in the slot (the lowest-row word is no longer needed);
//     voxel_inverse_kernel  every row reads the rank from its slot (skipped without an `inverse`).
//   Which slot a key lands in depends on who wins a CAS; nothing that is written out does: the representative is an integer
//   minimum, the population an integer sum, the order a prefix sum over row numbers.  The result is the same from run to run.
//
// This file is built with -ffp-contract=off: q = floor(((double)p - origin) / voxel) is two separately rounded fp64 operations.
#include "compact.h"
#include "slot_table.h"
#include "voxel_cell.h"

namespace {

constexpr int kThreads = 256;                                      // of the one-thread-per-row passes
constexpr int kNoRow = 0x7FFFFFFF;

struct alignas(16) Slot {
    unsigned long long key;
    int low;                                                        // the lowest row of the voxel; after voxel_write_kernel: its rank
    int pop;                                                        // valid rows in the voxel
};
static_assert(sizeof(Slot) == 16, "one slot is one 16-byte word");

template <bool kVec4>
__global__ __launch_bounds__(kThreads) void voxel_insert_kernel(const float *__restrict__ pts, int ld,
                                                                const int64_t *__restrict__ row_begin,
                                                                const int64_t *__restrict__ row_count, int max_rows, Grid grid,
                                                                Slot *__restrict__ table, unsigned cap, int *__restrict__ row_slot,
                                                                int64_t rows_pad, int *__restrict__ err) {
    const int b = blockIdx.y;
    const int n = pn2_clamped_rows(row_count, b, max_rows);
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
        unsigned long long key;
        if (pn2_cell_key_of(x, y, z, grid, key)) {
            Slot *tab = table + (int64_t)b * cap;
            slot = pn2_slot_claim(tab, cap - 1, key);
            if (slot >= 0) {                                        // (always: the cloud has at most cap / 2 rows)
                atomicMin(&tab[slot].low, i);
                atomicAdd(&tab[slot].pop, 1);
            }
        } else {
            dropped = true;
        }
        row_slot[(int64_t)b * rows_pad + i] = slot;
    }
    if (err != nullptr && __any(dropped) && (threadIdx.x & (PN2_WAVE - 1)) == 0) atomicOr(err, PN2_VOXEL_ERR_RANGE);
}

__global__ __launch_bounds__(kCompactThreads) void voxel_flag_kernel(const int64_t *__restrict__ row_count, int max_rows,
                                                                     const Slot *__restrict__ table, unsigned cap,
                                                                     const int *__restrict__ row_slot, unsigned char *__restrict__ flags,
                                                                     int *__restrict__ tile_count, int tiles) {
    const int b = blockIdx.y, tile = blockIdx.x;
    const int n = pn2_clamped_rows(row_count, b, max_rows);
    const int64_t t0 = (int64_t)tile * kCompactTile;
    if (t0 >= n) return;                                            // (uniform over the workgroup)
    const int64_t at = (int64_t)b * tiles + tile;
    const int *slot_of = row_slot + at * kCompactTile;
    const Slot *tab = table + (int64_t)b * cap;
    pn2_compact_flag_tile((int)(n - t0 < kCompactTile ? n - t0 : kCompactTile), flags + at * kCompactTile, tile_count + at, [&](int i) {
        const int s = slot_of[i];
        return s >= 0 && tab[s].low == (int)(t0 + i);
    });
}

template <bool kVec4>
__global__ __launch_bounds__(kCompactThreads) void voxel_write_kernel(const float *__restrict__ pts, int ld, const int32_t *__restrict__ labels_in,
                                                                      const int64_t *__restrict__ row_begin,
                                                                      const int64_t *__restrict__ row_count, int max_rows,
                                                                      Slot *__restrict__ table, unsigned cap, const int *__restrict__ row_slot,
                                                                      const unsigned char *__restrict__ flags,
                                                                      const int *__restrict__ tile_offset, int tiles,
                                                                      const int64_t *__restrict__ out_begin, float *__restrict__ out_points,
                                                                      int32_t *__restrict__ out_labels, int32_t *__restrict__ out_index,
                                                                      int32_t *__restrict__ n_points, int leave_rank) {
    const int b = blockIdx.y, tile = blockIdx.x;
    const int n = pn2_clamped_rows(row_count, b, max_rows);
    const int64_t t0 = (int64_t)tile * kCompactTile;
    if (t0 >= n) return;
    const int64_t base = row_begin[b] + t0, at = (int64_t)b * tiles + tile;
    const int *slot_of = row_slot + at * kCompactTile;
    const int first = tile_offset[at];                              // the rank, inside the cloud, of the tile's first representative
    const int64_t out0 = out_begin[b];
    Slot *tab = table + (int64_t)b * cap;
    pn2_compact_write_tile(flags + at * kCompactTile, [&](int i, int rank) {
        const int rk = first + rank;
        const int64_t o = out0 + rk;
        const int s = slot_of[i];
        if (out_points != nullptr) {
            if (kVec4) {
                reinterpret_cast<float4 *>(out_points)[o] = reinterpret_cast<const float4 *>(pts)[base + i];
            } else {
                const uint32_t *src = reinterpret_cast<const uint32_t *>(pts) + (base + i) * ld;
                uint32_t *dst = reinterpret_cast<uint32_t *>(out_points) + o * ld;
                for (int c = 0; c < ld; ++c) dst[c] = src[c];       // dword moves: the row bit for bit
            }
        }
        if (out_labels != nullptr) out_labels[o] = labels_in != nullptr ? labels_in[base + i] : 0;
        if (out_index != nullptr) out_index[o] = (int32_t)(t0 + i);
        if (n_points != nullptr) n_points[o] = tab[s].pop;
        if (leave_rank) tab[s].low = rk;                            // (nothing in this launch reads the word)
    });
}

__global__ __launch_bounds__(kThreads) void voxel_inverse_kernel(const int64_t *__restrict__ row_begin,
                                                                 const int64_t *__restrict__ row_count, int max_rows,
                                                                 const Slot *__restrict__ table, unsigned cap,
                                                                 const int *__restrict__ row_slot, int64_t rows_pad,
                                                                 int32_t *__restrict__ inverse) {
    const int b = blockIdx.y;
    const int n = pn2_clamped_rows(row_count, b, max_rows);
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int s = row_slot[(int64_t)b * rows_pad + i];
    inverse[row_begin[b] + i] = s >= 0 ? table[(int64_t)b * cap + s].low : -1;
}

// the workspace: the tables, a slot number per row of every tile, then the compaction's part
struct Work {
    Slot *table;
    int *row_slot;
    Pn2Compact compact;
    int64_t cap;                                                    // slots of one cloud's table
    int64_t bytes;
};

Work voxel_work(int B, int64_t max_rows, void *base) {
    Pn2Arena a(base);
    const int64_t cap = pn2_slot_capacity(max_rows);
    return {a.take<Slot>(B * cap), a.take<int>((int64_t)B * pn2_compact_tiles(max_rows) * kCompactTile), pn2_compact_take(a, B, max_rows), cap, a.bytes()};
}

}  // namespace

extern "C" {

int64_t pn2_voxel_grid_workspace_bytes(int B, int64_t max_rows) {
    return pn2_slot_shape_ok(B, max_rows) ? voxel_work(B, max_rows, nullptr).bytes : PN2_EINVAL;
}

int pn2_voxel_grid(const float *pts, int ld, const int32_t *labels_in, const int64_t *row_begin, const int64_t *row_count, int B,
                   int64_t max_rows, const double *origin, const double *voxel, const int64_t *out_begin, float *out_points,
                   int32_t *out_labels, int32_t *out_index, int64_t *out_count, int32_t *inverse, int32_t *n_points, int *err,
                   void *workspace, pn2_stream_t stream) {
    PN2_CHECK_ARG(pts && row_begin && row_count && origin && voxel && out_begin && out_count && workspace);
    PN2_CHECK_ARG(pn2_slot_shape_ok(B, max_rows) && ld >= 3 && ld <= 16);
    PN2_CHECK_ARG(pn2_aligned(pts, 4) && pn2_aligned(out_points, 4) && pn2_aligned(workspace, 16));
    Grid grid;
    PN2_CHECK_ARG(pn2_grid_from(origin, voxel, grid));
    const Work w = voxel_work(B, max_rows, workspace);
    const int tiles = w.compact.tiles;
    const int64_t cap = w.cap, rows_pad = (int64_t)tiles * kCompactTile, slots = (int64_t)B * cap;
    Slot *table = w.table;
    int *row_slot = w.row_slot;
    unsigned char *flags = w.compact.flags;
    int *tile_count = w.compact.tile_count, *tile_offset = w.compact.tile_offset;
    const bool vec4 = ld == 4 && pn2_aligned(pts, 16) && pn2_aligned(out_points, 16);
    const hipStream_t s = pn2_s(stream);
    const dim3 by_tile((unsigned)tiles, (unsigned)B), by_row((unsigned)(rows_pad / kThreads), (unsigned)B);
    hipLaunchKernelGGL(pn2_slot_clear_kernel, dim3(pn2_slot_clear_blocks(slots)), dim3(kSlotThreads), 0, s, reinterpret_cast<uint4 *>(table),
                       slots, pn2_slot_empty((unsigned)kNoRow, 0u));
    if (vec4)
        hipLaunchKernelGGL(voxel_insert_kernel<true>, by_row, dim3(kThreads), 0, s, pts, ld, row_begin, row_count, (int)max_rows, grid,
                           table, (unsigned)cap, row_slot, rows_pad, err);
    else
        hipLaunchKernelGGL(voxel_insert_kernel<false>, by_row, dim3(kThreads), 0, s, pts, ld, row_begin, row_count, (int)max_rows, grid,
                           table, (unsigned)cap, row_slot, rows_pad, err);
    hipLaunchKernelGGL(voxel_flag_kernel, by_tile, dim3(kCompactThreads), 0, s, row_count, (int)max_rows, table, (unsigned)cap, row_slot, flags,
                       tile_count, tiles);
    hipLaunchKernelGGL(pn2_compact_offsets_kernel, dim3((unsigned)B), dim3(PN2_WAVE), 0, s, row_count, (int)max_rows, tile_count,
                       tile_offset, tiles, out_count, err, PN2_VOXEL_ERR_ROWS);
    const int leave_rank = inverse != nullptr;
    if (out_points || out_labels || out_index || n_points || leave_rank) {
        if (vec4)
            hipLaunchKernelGGL(voxel_write_kernel<true>, by_tile, dim3(kCompactThreads), 0, s, pts, ld, labels_in, row_begin, row_count,
                               (int)max_rows, table, (unsigned)cap, row_slot, flags, tile_offset, tiles, out_begin, out_points, out_labels,
                               out_index, n_points, leave_rank);
        else
            hipLaunchKernelGGL(voxel_write_kernel<false>, by_tile, dim3(kCompactThreads), 0, s, pts, ld, labels_in, row_begin, row_count,
                               (int)max_rows, table, (unsigned)cap, row_slot, flags, tile_offset, tiles, out_begin, out_points, out_labels,
                               out_index, n_points, leave_rank);
    }
    if (leave_rank)
        hipLaunchKernelGGL(voxel_inverse_kernel, by_row, dim3(kThreads), 0, s, row_begin, row_count, (int)max_rows, table, (unsigned)cap,
                           row_slot, rows_pad, inverse);
    return pn2_launch_status();
}

}  // extern "C"
