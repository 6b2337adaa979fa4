// The persistent workspace pn2_grid_build fills (the slot table, the cell-sorted records, a word per row, a header per cloud) and the
// 27-cell walk over it, in ONE place: grid_knn.hip builds the workspace and searches it at K <= 32, icp.hip searches it at K = 1
// inside its accumulate kernel -- the two must agree on the layout to the byte and on the candidate set to the row.  Both files are
// built with -ffp-contract=off: the cell rule is two separately rounded fp64 operations, and the distance is pn2_chamfer_nn's
// difference form at D = 3 with its two fused steps spelled __builtin_fmaf.
#pragma once
#include "knn_select.h"
#include "slot_table.h"
#include "voxel_cell.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 4;                                       // slots per thread of the two tile kernels
constexpr int kTile = kThreads * kPerThread;                        // slots per workgroup of the two tile kernels
constexpr int kWaves = kThreads / PN2_WAVE;

struct alignas(16) Slot {
    unsigned long long key;
    int next;                                                       // after the scan: the cell's first record; the fill advances it past the last
    int pop;                                                        // candidates in the cell
};
static_assert(sizeof(Slot) == 16, "one slot is one 16-byte word");

struct alignas(16) Head {                                           // per cloud
    int count;                                                      // candidate rows the build read (clamped n_cand)
    int indexed;                                                    // of them in the grid: records [0, indexed) are the cells'
    int tail;                                                       // cursor of the rows that are not: records [indexed, count)
    int unused;
};

struct Work {
    Slot *table;
    float4 *rec;
    int *row_word;                                                  // per row: its slot between count and fill, its record's position afterwards
    int *tile_sum, *tile_start;
    Head *head;
    unsigned cap;                                                   // slots of one cloud's table
    int tiles;                                                      // per cloud
};

// The workspace: the tables, the records, a word per row, two words per tile of slots, a header per cloud.
Work grid_work(int B, int64_t M, void *base, int64_t *bytes = nullptr) {
    Pn2Arena a(base);
    const int64_t cap = pn2_slot_capacity(M), tiles = pn2_cdiv(cap, kTile);
    const Work w{a.take<Slot>(B * cap),   a.take<float4>(B * M), a.take<int>(B * M), a.take<int>(B * tiles),
                 a.take<int>(B * tiles), a.take<Head>(B),       (unsigned)cap,      (int)tiles};
    if (bytes != nullptr) *bytes = a.bytes();
    return w;
}

bool grid_shape_ok(int B, int64_t M) { return pn2_slot_shape_ok(B, M) && M >= 1; }

// One lane's walk over the 27 cells around the query (qx, qy, qz) of cloud b: every indexed candidate of those cells with
// d2 <= max_d2 is counted in `took` and offered to the lane's CAP best pairs (knn_select.h; the caller set them to (+inf, M)).
// false: the query is not finite or lies outside the grid, nothing was walked.  Everything read from the workspace that is used as
// an address is checked against M first: a workspace that no build filled cannot send a lane out of bounds.
template <int CAP>
__device__ __forceinline__ bool pn2_grid_walk(float qx, float qy, float qz, const Grid &grid, const Work &w, int b, int M, float max_d2,
                                              float (&bd)[CAP], int (&bi)[CAP], int &took) {
    unsigned long long cx, cy, cz;
    if (!(cell_of(qx, grid.origin[0], grid.voxel[0], cx) && cell_of(qy, grid.origin[1], grid.voxel[1], cy) &&
          cell_of(qz, grid.origin[2], grid.voxel[2], cz)))
        return false;
    const float4 *__restrict__ rec = w.rec + (int64_t)b * M;
    const Slot *__restrict__ tab = w.table + (int64_t)b * w.cap;
#pragma nounroll
    for (int c = 0; c < 27; ++c) {
        // the neighbour's cell, per axis BEFORE the key is formed: cells at the two ends of an axis differ by 1 in the packed word
        const long long nx = (long long)cx + (c / 9 - 1), ny = (long long)cy + (c / 3 % 3 - 1), nz = (long long)cz + (c % 3 - 1);
        if (nx < 0 || nx >= kCells || ny < 0 || ny >= kCells || nz < 0 || nz >= kCells) continue;
        const int slot = pn2_slot_find(tab, w.cap - 1u, pn2_cell_key((unsigned long long)nx, (unsigned long long)ny, (unsigned long long)nz));
        if (slot < 0) continue;
        const uint4 cell = reinterpret_cast<const uint4 *>(tab)[slot];
        const int next = (int)cell.z, pop = (int)cell.w;
        const int hi = next < M ? next : M;
        int k = next - pop;
        k = k > 0 ? k : 0;
        for (; k < hi; ++k) {
            const float4 r = rec[k];
            int j = __float_as_int(r.w);
            PN2_OPAQUE1(j);                                     // (used on every trip: the record stays ONE 16-byte load, its index is not fetched again inside the branch)
            const float tx = qx - r.x, ty = qy - r.y, tz = qz - r.z;
            float d2 = tx * tx;
            d2 = __builtin_fmaf(ty, ty, d2);
            d2 = __builtin_fmaf(tz, tz, d2);
            if (d2 <= max_d2) {                                 // (a NaN fails)
                ++took;
                pn2_select_insert<CAP>(bd, bi, d2, j);
            }
        }
    }
    return true;
}

}  // namespace
