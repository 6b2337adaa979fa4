// Euclidean clustering on the voxel grid: connected components of the occupied cells of a pn2_voxel_grid result, for a batch of
// clouds, with the component COUNT left in device memory, ids in ascending order of the components' lowest voxel (a STABLE
// compaction again) and an `inverse`-style map from every row to its component.  The rule is in include/pn2.h.
//
//   pn2_voxel_components   eight plain launches on the caller's stream, no thread ever waits for another thread's write:
//     cluster_clear_kernel   every slot of every cloud's table (slot_table.h) to EMPTY, parent[v] = v, the two per-root counters 0;
//     cluster_insert_kernel  one thread per voxel: does it take part, the cell key of its representative row (fp64, the rule of
//                            voxel_cell.h), pn2_slot_claim, the voxel's rank as the payload; the key is remembered per voxel;
//     cluster_link_kernel    a LATER launch, one thread per (voxel, half-neighbour): the 3, 9 or 13 offsets whose first non-zero
//                            entry is +1 (the other half is the neighbour's job), a read-only probe (pn2_slot_find), then a
//                            lock-free union on parent[].  INVARIANT: parent[x] <= x, and parent[x] lies in x's component.  Every
//                            write is an atomicMin of a non-root towards an ancestor or an atomicCAS that links a root to a lower
//                            voxel of the other tree; entries only ever decrease, so every loop terminates, and a walk is capped
//                            by the cloud's voxel count all the same (PN2_CLUSTER_ERR_CAP: the thread stops, it does not spin);
//     cluster_flatten_kernel a LATER launch: root[v] into its own array, n_points[v] and 1 added to the root's counters;
//     cluster_flag_kernel / pn2_compact_offsets_kernel / cluster_write_kernel   the stable compaction of compact.h over "v is a
//                            root, takes part and its component is kept"; the write pass stores the four per-component outputs and
//                            leaves the id in parent[root] (the forest is no longer needed);
//     cluster_assign_kernel  per voxel and per row: the id of the root, -1 for none.
//   Which links the races make differs from run to run; what is written out does not: the partition is a property of the graph,
//   the root of a part is an integer minimum (the one voxel of the part that cannot have a parent below it), the counters are
//   integer sums and the ids are prefix sums over ranks.  The result is the same from run to run.
//
// This file is built with -ffp-contract=off: q = floor(((double)p - origin) / voxel) is two separately rounded fp64 operations.
#include "compact.h"
#include "slot_table.h"
#include "voxel_cell.h"

namespace {

constexpr int kThreads = 256;
constexpr int kNoRank = 0x7FFFFFFF;

struct alignas(16) Slot {
    unsigned long long key;
    int rank;                                                       // the voxel that lies in this cell
    int unused;
};
static_assert(sizeof(Slot) == 16, "one slot is one 16-byte word");

struct Rule {
    int half;                                                       // half-neighbours per voxel: 3, 9 or 13
    int same_label, L, min_points, min_voxels;
};

// The 13 offsets whose first non-zero entry is +1, sorted by their number of non-zero entries: the first 3 are the half of
// connectivity 6, the first 9 of 18, all 13 of 26.  Packed two bits per axis (d + 1), x in the high bits.
__device__ __forceinline__ void half_offset(int h, int &dx, int &dy, int &dz) {
    //                               1 entry: +x +y +z      2 entries: (1,1,0) (1,-1,0) (1,0,1) (1,0,-1) (0,1,1) (0,1,-1)      3 entries: (1,+-1,+-1)
    const unsigned long long lo = 0x1A24262129161925ull, hi = 0x20222A2818ull;          // a byte per offset, two words: no memory
    const unsigned code = (unsigned)((h < 8 ? lo >> (8 * h) : hi >> (8 * (h - 8))) & 0xFFu);
    dx = (int)((code >> 4) & 3u) - 1;
    dy = (int)((code >> 2) & 3u) - 1;
    dz = (int)(code & 3u) - 1;
}

__device__ __forceinline__ int load_parent(const int *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

// The root of x's tree at some moment of this call, halving the path on the way: x's entry moves to its grandparent through an
// atomicMin (x is no root: only a root's entry is ever compared-and-swapped, so the two kinds of write never meet on one word).
// Entries strictly decrease along a path, so a walk takes fewer than `cap` (the cloud's voxel count) steps; -1 when it took more.
__device__ __forceinline__ int find_root(int *parent, int x, int cap) {
    for (int step = 0; step <= cap; ++step) {
        const int p = load_parent(parent + x);
        if (p == x) return x;
        const int g = load_parent(parent + p);
        if (g == p) return p;
        atomicMin(parent + x, g);
        x = g;
    }
    return -1;
}

// Joins the trees of a and b.  A failed compare-and-swap means the higher root got a parent meanwhile: the walk goes on from there,
// strictly below, so there are fewer than `cap` rounds.  false: a cap was hit.
__device__ __forceinline__ bool unite(int *parent, int a, int b, int cap) {
    for (int round = 0; round <= cap; ++round) {
        a = find_root(parent, a, cap);
        b = find_root(parent, b, cap);
        if (a < 0 || b < 0) return false;
        if (a == b) return true;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int seen = atomicCAS(parent + hi, hi, lo);
        if (seen == hi) return true;
        a = seen;                                                   // (< hi: hi's new parent)
        b = lo;
    }
    return false;
}

struct Work {
    Slot *table;
    unsigned long long *key;                                        // per voxel: its cell key, EMPTY when it takes no part
    int *parent, *root, *points, *voxels;                           // per voxel; points / voxels: the counters of a root
    unsigned char *flags;
    int *tile_count, *tile_offset;
    unsigned cap;                                                   // slots of one cloud's table as allocated
    int tiles;
    int64_t pad;                                                    // entries per cloud of the per-voxel arrays
};

// The workspace: the tables; per voxel of every tile its key, parent, root and the two counters; then the compaction's part.
Work cluster_work(int B, int64_t max_rows, void *base, int64_t *bytes = nullptr) {
    Pn2Arena a(base);
    const int64_t cap = pn2_slot_capacity(max_rows), pad = (int64_t)pn2_compact_tiles(max_rows) * kCompactTile, n = B * pad;
    Slot *table = a.take<Slot>(B * cap);
    unsigned long long *key = a.take<unsigned long long>(n);
    int *parent = a.take<int>(n), *root = a.take<int>(n), *points = a.take<int>(n), *voxels = a.take<int>(n);
    const Pn2Compact c = pn2_compact_take(a, B, max_rows);
    if (bytes != nullptr) *bytes = a.bytes();
    return {table, key, parent, root, points, voxels, c.flags, c.tile_count, c.tile_offset, (unsigned)cap, c.tiles, pad};
}

__global__ __launch_bounds__(kThreads) void cluster_clear_kernel(const int64_t *__restrict__ out_count, int max_rows, Work w) {
    const int b = blockIdx.y;
    const int nv = pn2_clamped_rows(out_count, b, max_rows);
    const int64_t used = pn2_slot_capacity(nv);                     // <= w.cap: the rule is monotone
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < used) reinterpret_cast<uint4 *>(w.table + (int64_t)b * w.cap)[i] = pn2_slot_empty((unsigned)kNoRank, 0u);
    if (i < nv) {
        const int64_t at = (int64_t)b * w.pad + i;
        w.parent[at] = (int)i;
        w.points[at] = 0;
        w.voxels[at] = 0;
    }
}

__global__ __launch_bounds__(kThreads) void cluster_insert_kernel(const float *__restrict__ pts, int ld, const int64_t *__restrict__ row_begin,
                                                                  const int64_t *__restrict__ row_count, const int64_t *__restrict__ out_begin,
                                                                  const int64_t *__restrict__ out_count, int max_rows, Grid grid,
                                                                  const int32_t *__restrict__ out_index, const int32_t *__restrict__ vox_labels,
                                                                  const int32_t *__restrict__ member, Rule rule, Work w, int *__restrict__ err) {
    const int b = blockIdx.y;
    const int nv = pn2_clamped_rows(out_count, b, max_rows);
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if ((int64_t)blockIdx.x * kThreads >= nv) return;               // (uniform over the workgroup)
    int bits = 0;
    if (i < nv) {
        const int v = (int)i;
        const int64_t o = out_begin[b] + v;
        bool part = true;
        if (vox_labels != nullptr) {
            const int32_t lab = vox_labels[o];
            part = lab >= 0 && (member == nullptr || (lab < rule.L && member[lab] != 0));
        }
        unsigned long long key = kEmpty;
        if (part) {
            const int32_t r = out_index[o];
            if (r < 0 || r >= pn2_clamped_rows(row_count, b, max_rows)) {
                bits = PN2_CLUSTER_ERR_INDEX;                        // skipped, never addressed
            } else {
                const float *p = pts + (row_begin[b] + r) * ld;
                if (pn2_cell_key_of(p[0], p[1], p[2], grid, key)) {
                    Slot *tab = w.table + (int64_t)b * w.cap;
                    const int slot = pn2_slot_claim(tab, (unsigned)pn2_slot_capacity(nv) - 1u, key);
                    // (one writer per slot: a grid's voxels have distinct cells.  The minimum keeps a malformed input, two voxels
                    // in one cell, deterministic: the lower one stands for the cell, the other has no neighbours of its own.)
                    if (slot >= 0) atomicMin(&tab[slot].rank, v);
                } else {
                    bits = PN2_CLUSTER_ERR_CELL;
                }
            }
        }
        w.key[(int64_t)b * w.pad + v] = key;
    }
    if (err != nullptr && bits != 0) atomicOr(err, bits);
}

__global__ __launch_bounds__(kThreads) void cluster_link_kernel(const int64_t *__restrict__ out_begin, const int64_t *__restrict__ out_count,
                                                                int max_rows, const int32_t *__restrict__ vox_labels, Rule rule, Work w,
                                                                int *__restrict__ err) {
    const int b = blockIdx.y;
    const int nv = pn2_clamped_rows(out_count, b, max_rows);
    const int64_t v64 = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v64 >= nv) return;
    const int v = (int)v64, h = blockIdx.z;                         // (adjacent lanes: adjacent voxels, one offset)
    const unsigned long long key = w.key[(int64_t)b * w.pad + v];
    if (key == kEmpty) return;
    int dx, dy, dz;
    half_offset(h, dx, dy, dz);
    // the neighbour's cell, per axis BEFORE the key is formed: cells at the two ends of an axis differ by 1 in the packed word
    const long long nx = (long long)(key >> 42) + dx, ny = (long long)((key >> 21) & (kCells - 1)) + dy,
                    nz = (long long)(key & (kCells - 1)) + dz;
    if (nx < 0 || nx >= kCells || ny < 0 || ny >= kCells || nz < 0 || nz >= kCells) return;
    const unsigned long long other = pn2_cell_key((unsigned long long)nx, (unsigned long long)ny, (unsigned long long)nz);
    const Slot *tab = w.table + (int64_t)b * w.cap;
    const int slot = pn2_slot_find(tab, (unsigned)pn2_slot_capacity(nv) - 1u, other);
    if (slot < 0) return;
    const int u = tab[slot].rank;
    if (u < 0 || u >= nv || u == v) return;                         // (never: ranks are below the count)
    if (rule.same_label && vox_labels != nullptr) {
        const int64_t o = out_begin[b];
        if (vox_labels[o + v] != vox_labels[o + u]) return;
    }
    if (!unite(w.parent + (int64_t)b * w.pad, v, u, nv) && err != nullptr) atomicOr(err, PN2_CLUSTER_ERR_CAP);
}

__global__ __launch_bounds__(kThreads) void cluster_flatten_kernel(const int64_t *__restrict__ out_begin, const int64_t *__restrict__ out_count,
                                                                   int max_rows, const int32_t *__restrict__ n_points, Work w,
                                                                   int *__restrict__ err) {
    const int b = blockIdx.y;
    const int nv = pn2_clamped_rows(out_count, b, max_rows);
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= nv) return;
    const int64_t base = (int64_t)b * w.pad;
    int r = -1;
    if (w.key[base + i] != kEmpty) {
        r = find_root(w.parent + base, (int)i, nv);
        if (r < 0) {
            if (err != nullptr) atomicOr(err, PN2_CLUSTER_ERR_CAP);
        } else {
            atomicAdd(w.points + base + r, n_points[out_begin[b] + i]);
            atomicAdd(w.voxels + base + r, 1);
        }
    }
    w.root[base + i] = r;
}

__global__ __launch_bounds__(kCompactThreads) void cluster_flag_kernel(const int64_t *__restrict__ out_count, int max_rows, Rule rule, Work w) {
    const int b = blockIdx.y, tile = blockIdx.x;
    const int nv = pn2_clamped_rows(out_count, b, max_rows);
    const int64_t t0 = (int64_t)tile * kCompactTile;
    if (t0 >= nv) return;                                           // (uniform over the workgroup)
    const int64_t at = (int64_t)b * w.tiles + tile;
    const int *root = w.root + at * kCompactTile, *points = w.points + at * kCompactTile, *voxels = w.voxels + at * kCompactTile;
    pn2_compact_flag_tile((int)(nv - t0 < kCompactTile ? nv - t0 : kCompactTile), w.flags + at * kCompactTile, w.tile_count + at, [&](int i) {
        return root[i] == (int)(t0 + i) && points[i] >= rule.min_points && voxels[i] >= rule.min_voxels;
    });
}

__global__ __launch_bounds__(kCompactThreads) void cluster_write_kernel(const int64_t *__restrict__ out_begin, const int64_t *__restrict__ out_count,
                                                                        int max_rows, const int32_t *__restrict__ vox_labels,
                                                                        const int64_t *__restrict__ comp_begin, int32_t *__restrict__ comp_root,
                                                                        int32_t *__restrict__ comp_points, int32_t *__restrict__ comp_voxels,
                                                                        int32_t *__restrict__ comp_label, Work w) {
    const int b = blockIdx.y, tile = blockIdx.x;
    const int nv = pn2_clamped_rows(out_count, b, max_rows);
    const int64_t t0 = (int64_t)tile * kCompactTile;
    if (t0 >= nv) return;
    const int64_t at = (int64_t)b * w.tiles + tile;
    const int first = w.tile_offset[at];                            // the id of the tile's first kept root
    const int64_t c0 = comp_begin[b], v0 = out_begin[b] + t0;
    int *parent = w.parent + at * kCompactTile;
    const int *points = w.points + at * kCompactTile, *voxels = w.voxels + at * kCompactTile;
    pn2_compact_write_tile(w.flags + at * kCompactTile, [&](int i, int rank) {
        const int id = first + rank;
        const int64_t o = c0 + id;
        if (comp_root != nullptr) comp_root[o] = (int32_t)(t0 + i);
        if (comp_points != nullptr) comp_points[o] = points[i];
        if (comp_voxels != nullptr) comp_voxels[o] = voxels[i];
        if (comp_label != nullptr) comp_label[o] = vox_labels != nullptr ? vox_labels[v0 + i] : 0;
        parent[i] = id;                                             // (nothing in this launch reads the word)
    });
}

__global__ __launch_bounds__(kThreads) void cluster_assign_kernel(const int64_t *__restrict__ row_begin, const int64_t *__restrict__ row_count,
                                                                  const int64_t *__restrict__ out_begin, const int64_t *__restrict__ out_count,
                                                                  int max_rows, const int32_t *__restrict__ vox_labels,
                                                                  const int32_t *__restrict__ inverse, const int32_t *__restrict__ row_labels,
                                                                  int32_t *__restrict__ vox_component, int32_t *__restrict__ row_component,
                                                                  Work w, int *__restrict__ err) {
    const int b = blockIdx.y;
    const int nv = pn2_clamped_rows(out_count, b, max_rows);
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t base = (int64_t)b * w.pad;
    const auto id_of = [&](int v) {
        const int r = w.root[base + v];
        return r >= 0 && w.flags[base + r] != 0 ? w.parent[base + r] : -1;
    };
    if (vox_component != nullptr && i < nv) vox_component[out_begin[b] + i] = id_of((int)i);
    if (row_component != nullptr) {
        const int n = pn2_clamped_rows(row_count, b, max_rows);
        if (i < n) {
            const int64_t row = row_begin[b] + i;
            const int32_t v = inverse[row];
            int id = -1;
            if (v >= nv) {
                if (err != nullptr) atomicOr(err, PN2_CLUSTER_ERR_INDEX);
            } else if (v >= 0 && (row_labels == nullptr || row_labels[row] == vox_labels[out_begin[b] + v])) {
                id = id_of(v);
            }
            row_component[row] = id;
        }
        if (i == 0 && err != nullptr && row_count[b] > max_rows) atomicOr(err, PN2_CLUSTER_ERR_ROWS);
    }
}

}  // namespace

extern "C" {

int64_t pn2_voxel_components_workspace_bytes(int B, int64_t max_rows) {
    int64_t bytes = PN2_EINVAL;
    if (pn2_slot_shape_ok(B, max_rows)) cluster_work(B, max_rows, nullptr, &bytes);
    return bytes;
}

int pn2_voxel_components(const float *pts, int ld, const int64_t *row_begin, const int64_t *row_count, int B, int64_t max_rows,
                         const double *origin, const double *voxel, const int64_t *out_begin, const int64_t *out_count,
                         const int32_t *out_index, const int32_t *n_points, const int32_t *vox_labels, const int32_t *inverse,
                         const int32_t *row_labels, int connectivity, int same_label, const int32_t *member, int L, int min_points,
                         int min_voxels, const int64_t *comp_begin, int32_t *vox_component, int32_t *row_component, int32_t *comp_root,
                         int32_t *comp_points, int32_t *comp_voxels, int32_t *comp_label, int64_t *comp_count, int *err, void *workspace,
                         pn2_stream_t stream) {
    PN2_CHECK_ARG(pts && row_begin && row_count && origin && voxel && out_begin && out_count && out_index && n_points && comp_begin &&
                  comp_count && workspace);
    PN2_CHECK_ARG(pn2_slot_shape_ok(B, max_rows) && ld >= 3 && ld <= 16);
    PN2_CHECK_ARG(connectivity == 6 || connectivity == 18 || connectivity == 26);
    PN2_CHECK_ARG(min_points >= 1 && min_voxels >= 1);
    PN2_CHECK_ARG(member == nullptr || (vox_labels != nullptr && L >= 1));
    PN2_CHECK_ARG(row_labels == nullptr || vox_labels != nullptr);
    PN2_CHECK_ARG(row_component == nullptr || inverse != nullptr);
    PN2_CHECK_ARG(pn2_aligned(pts, 4) && pn2_aligned(workspace, 16));
    Grid grid;
    PN2_CHECK_ARG(pn2_grid_from(origin, voxel, grid));
    Rule rule;
    rule.half = connectivity == 6 ? 3 : (connectivity == 18 ? 9 : 13);
    rule.same_label = same_label != 0;
    rule.L = member != nullptr ? L : 0;
    rule.min_points = min_points;
    rule.min_voxels = min_voxels;
    const Work w = cluster_work(B, max_rows, workspace);
    const hipStream_t s = pn2_s(stream);
    const dim3 by_tile((unsigned)w.tiles, (unsigned)B), by_row((unsigned)(w.pad / kThreads), (unsigned)B);
    const dim3 by_slot((unsigned)pn2_cdiv((int64_t)w.cap > w.pad ? (int64_t)w.cap : w.pad, kThreads), (unsigned)B);
    const dim3 by_pair((unsigned)(w.pad / kThreads), (unsigned)B, (unsigned)rule.half);
    hipLaunchKernelGGL(cluster_clear_kernel, by_slot, dim3(kThreads), 0, s, out_count, (int)max_rows, w);
    hipLaunchKernelGGL(cluster_insert_kernel, by_row, dim3(kThreads), 0, s, pts, ld, row_begin, row_count, out_begin, out_count, (int)max_rows,
                       grid, out_index, vox_labels, member, rule, w, err);
    hipLaunchKernelGGL(cluster_link_kernel, by_pair, dim3(kThreads), 0, s, out_begin, out_count, (int)max_rows, vox_labels, rule, w, err);
    hipLaunchKernelGGL(cluster_flatten_kernel, by_row, dim3(kThreads), 0, s, out_begin, out_count, (int)max_rows, n_points, w, err);
    hipLaunchKernelGGL(cluster_flag_kernel, by_tile, dim3(kCompactThreads), 0, s, out_count, (int)max_rows, rule, w);
    hipLaunchKernelGGL(pn2_compact_offsets_kernel, dim3((unsigned)B), dim3(PN2_WAVE), 0, s, out_count, (int)max_rows, w.tile_count,
                       w.tile_offset, w.tiles, comp_count, err, PN2_CLUSTER_ERR_ROWS);
    hipLaunchKernelGGL(cluster_write_kernel, by_tile, dim3(kCompactThreads), 0, s, out_begin, out_count, (int)max_rows, vox_labels, comp_begin,
                       comp_root, comp_points, comp_voxels, comp_label, w);
    if (vox_component != nullptr || row_component != nullptr)
        hipLaunchKernelGGL(cluster_assign_kernel, by_row, dim3(kThreads), 0, s, row_begin, row_count, out_begin, out_count, (int)max_rows,
                           vox_labels, inverse, row_labels, vox_component, row_component, w, err);
    return pn2_launch_status();
}

}  // extern "C"
