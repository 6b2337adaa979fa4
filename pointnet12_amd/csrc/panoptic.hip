// Panoptic quality of instance labels (include/pn2.h, "panoptic quality"): per class the matches (tp), the unmatched predicted and
// ground-truth segments (fp, fn) and the sum of the matches' IoU, for a batch of clouds whose rows carry (pred_sem, pred_inst, gt_sem,
// gt_inst).  Everything the scores need follows from INTEGER counts per (class, instance) pair, and everything that crosses threads is
// an integer atomic (compare-and-swap on a key, add): integer sums commute, so the table is the same from run to run, byte for byte,
// whatever the order of the rows' arrival, the hash layout, the wave combining or the grid shape -- no sort, no read-back per scan.
//
//   pn2_panoptic_count   four plain launches on the caller's stream, a launch boundary is the only ordering:
//     clear_kernel     the slots in use of the cloud's three tables (slot_table.h, capacity of the device-side row count) to empty;
//     count_kernel     one thread per row: claims the row's ground-truth segment (key class << 32 | id) and predicted segment (the
//                      same) and adds to their areas; where both exist and the classes agree it claims the pair (key gt slot << 32 |
//                      pred slot: pn2_slot_claim hands the slot back at once) and adds to its intersection;
//     match_kernel     one thread per pair slot: the areas are final, 2 * inter > union on integers; a match sets both segments'
//                      flags (every writer stores the same 1, and a segment matches at most once: two disjoint overlaps cannot both
//                      exceed half of it), adds tp and the two halves of the IoU's 53-bit integer;
//     residue_kernel   one thread per segment slot of both tables: unmatched with area >= min_points adds fn / fp.
//   A scan's road is ONE segment of tens of thousands of rows: the lanes of a wave that hold the same key are found with ballots
//   (pn2_wave_combine, kRounds leaders; whatever is left goes lane by lane), ONE lane claims the slot and adds the
//   count of its voters, and hands the slot to them with a shuffle.  The match and residue launches do the same per class.
//   -DPN2_PANOPTIC_COMBINE=0 (make XFLAGS=...) builds the uncombined form for measurements; integer addition is associative: the bytes
//   are the same either way.  No thread waits for another thread's write; every probe loop is bounded by its table.
//
// This file is built with -ffp-contract=off: the IoU is ONE IEEE fp64 division, scaled by an exact power of two.
#include "slot_table.h"
#include "wave_ops.h"

#ifndef PN2_PANOPTIC_COMBINE
#define PN2_PANOPTIC_COMBINE 1
#endif

namespace {

constexpr int kThreads = 256;
constexpr bool kCombine = PN2_PANOPTIC_COMBINE != 0;
constexpr int kRounds = 4;                                          // keys a wave combines with ballots before its lanes go alone
constexpr int kColumns = 5;                                         // tp, fp, fn, iou_hi, iou_lo
static_assert(kThreads == kSlotThreads, "clear_kernel fills its tables with pn2_slot_fill; the grids come from pn2_slot_blocks");

struct alignas(16) Slot {
    unsigned long long key;                                         // segments: class << 32 | id; pairs: gt slot << 32 | pred slot
    int count;                                                      // segments: the area; pairs: the intersection
    int matched;                                                    // segments: 1 once a pair matched it
};
static_assert(sizeof(Slot) == 16, "one slot is one 16-byte word");

// Rows of cloud b (the device-side count clamped to [0, max_rows]) and where they begin; -1 when they would leave the buffers' `rows`
// rows: such a cloud is skipped whole by every launch.
__device__ __forceinline__ int cloud_rows(const int64_t *__restrict__ row_begin, const int64_t *__restrict__ row_count, int b,
                                          int max_rows, int64_t rows, int64_t &begin) {
    const int n = pn2_clamped_rows(row_count, b, max_rows);
    begin = row_begin[b];
    return begin < 0 || begin > rows - n ? -1 : n;
}

// The slot of `key` for every lane that is `live` (-1 for the others), its counter raised by one per such lane.  Called by whole waves.
__device__ __forceinline__ int claim_and_add(Slot *table, unsigned mask, unsigned long long key, bool live) {
    int slot = -1;
    if (kCombine) {
        const int lane = threadIdx.x & (PN2_WAVE - 1);
        live = pn2_wave_combine<kRounds>(key, live, [&](bool voter, int leader, unsigned long long votes) {
            int s = -1;
            if (lane == leader) {
                s = pn2_slot_claim(table, mask, key);
                if (s >= 0) atomicAdd(&table[s].count, __popcll(votes));
            }
            s = __shfl(s, leader, PN2_WAVE);
            if (voter) slot = s;
        });
    }
    if (live) {
        slot = pn2_slot_claim(table, mask, key);                    // (never -1: a table holds at most as many keys as the cloud has rows)
        if (slot >= 0) atomicAdd(&table[slot].count, 1);
    }
    return slot;
}

__device__ __forceinline__ void add_i64(int64_t *word, unsigned long long value) {
    atomicAdd(reinterpret_cast<unsigned long long *>(word), value);
}

__global__ __launch_bounds__(kThreads) void clear_kernel(const int64_t *__restrict__ row_begin, const int64_t *__restrict__ row_count,
                                                         int max_rows, int64_t rows, uint4 *__restrict__ tables, int64_t cap) {
    const int b = blockIdx.y;
    int64_t begin;
    const int n = cloud_rows(row_begin, row_count, b, max_rows, rows, begin);
    if (n < 0) return;
    const int64_t used = pn2_slot_capacity(n);                      // the slots in USE: <= cap
    for (int t = 0; t < 3; ++t) pn2_slot_fill(tables + ((int64_t)b * 3 + t) * cap, used, pn2_slot_empty(0u, 0u));
}

__global__ __launch_bounds__(kThreads) void count_kernel(const int32_t *__restrict__ pred_sem, const int32_t *__restrict__ pred_inst,
                                                         const int32_t *__restrict__ gt_sem, const int32_t *__restrict__ gt_inst,
                                                         const int64_t *__restrict__ row_begin, const int64_t *__restrict__ row_count,
                                                         int max_rows, int64_t rows, int C, const int32_t *__restrict__ include,
                                                         const int32_t *__restrict__ things, Slot *tables, int64_t cap,
                                                         int *__restrict__ err) {
    const int b = blockIdx.y;
    int64_t begin;
    const int n = cloud_rows(row_begin, row_count, b, max_rows, rows, begin);
    if (n < 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && err != nullptr) atomicOr(err, PN2_PANOPTIC_ERR_ROWS);
        return;
    }
    if ((int64_t)blockIdx.x * kThreads >= n) return;                // (uniform over the workgroup)
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    bool has_gt = false, has_pred = false, bad = false;
    unsigned long long gt_key = 0ull, pred_key = 0ull;
    int gs = -1, ps = -1;
    if (i < n) {
        const int64_t row = begin + i;
        gs = gt_sem[row];
        if (gs < 0 || gs >= C) {
            bad = true;                                             // no class: the row is dropped from both sides
        } else if (include[gs] != 0) {
            int gi = gt_inst[row], pi = pred_inst[row];
            ps = pred_sem[row];
            const bool pred_class = ps >= 0 && ps < C && include[ps] != 0;
            if (things != nullptr) {                                // a stuff class is one segment: its ids count as 0
                if (things[gs] == 0) gi = 0;
                if (pred_class && things[ps] == 0) pi = 0;
            }
            has_gt = gi >= 0;
            has_pred = pred_class && pi >= 0;
            gt_key = ((unsigned long long)(unsigned)gs << 32) | (unsigned)gi;
            pred_key = ((unsigned long long)(unsigned)ps << 32) | (unsigned)pi;
        }
    }
    Slot *gt = tables + (int64_t)b * 3 * cap, *pred = gt + cap, *pairs = pred + cap;
    const unsigned mask = (unsigned)pn2_slot_capacity(n) - 1u;
    const int gt_slot = claim_and_add(gt, mask, gt_key, has_gt);
    const int pred_slot = claim_and_add(pred, mask, pred_key, has_pred);
    const bool both = gt_slot >= 0 && pred_slot >= 0 && gs == ps;
    claim_and_add(pairs, mask, ((unsigned long long)(unsigned)gt_slot << 32) | (unsigned)pred_slot, both);
    if (err != nullptr && __any(bad) && (threadIdx.x & (PN2_WAVE - 1)) == 0) atomicOr(err, PN2_PANOPTIC_ERR_CLASS);
}

__global__ __launch_bounds__(kThreads) void match_kernel(const int64_t *__restrict__ row_begin, const int64_t *__restrict__ row_count,
                                                         int max_rows, int64_t rows, Slot *tables, int64_t cap, int64_t *out,
                                                         int64_t out_stride) {
    const int b = blockIdx.y;
    int64_t begin;
    const int n = cloud_rows(row_begin, row_count, b, max_rows, rows, begin);
    if (n < 0) return;
    const int64_t used = pn2_slot_capacity(n);
    if ((int64_t)blockIdx.x * kThreads >= used) return;             // (uniform over the workgroup)
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    Slot *gt = tables + (int64_t)b * 3 * cap, *pred = gt + cap;
    const Slot *pairs = pred + cap;
    bool live = false;
    unsigned cls = 0u;
    unsigned long long hi = 0ull, lo = 0ull;
    if (i < used) {
        const Slot p = pairs[i];
        if (p.key != kEmpty) {
            const unsigned g = (unsigned)(p.key >> 32), q = (unsigned)p.key;
            const int64_t inter = p.count, uni = (int64_t)gt[g].count + (int64_t)pred[q].count - inter;     // (final: a launch ago)
            if (2 * inter > uni) {
                gt[g].matched = 1;
                pred[q].matched = 1;
                cls = (unsigned)(gt[g].key >> 32);
                const double iou = (double)inter / (double)uni;     // ONE IEEE division, in (0.5, 1]
                const unsigned long long t = (unsigned long long)(iou * 9007199254740992.0);     // * 2^53: exact, an integer
                hi = t >> 32;
                lo = t & 0xFFFFFFFFull;
                live = true;
            }
        }
    }
    int64_t *dst = out + (int64_t)b * out_stride;
    if (kCombine) {                                                 // the matches of one class in this wave are added by one lane
        const int lane = threadIdx.x & (PN2_WAVE - 1);              // (most waves hold no match at all)
        live = pn2_wave_combine<kRounds>(cls, live, [&](bool voter, int leader, unsigned long long votes) {
            const unsigned long long sum_hi = pn2_wave_sum_u64(voter ? hi : 0ull), sum_lo = pn2_wave_sum_u64(voter ? lo : 0ull);
            if (lane == leader) {
                add_i64(dst + (int64_t)cls * kColumns + 0, (unsigned long long)__popcll(votes));
                add_i64(dst + (int64_t)cls * kColumns + 3, sum_hi);
                add_i64(dst + (int64_t)cls * kColumns + 4, sum_lo);
            }
        });
    }
    if (live) {
        add_i64(dst + (int64_t)cls * kColumns + 0, 1ull);
        add_i64(dst + (int64_t)cls * kColumns + 3, hi);
        add_i64(dst + (int64_t)cls * kColumns + 4, lo);
    }
}

__global__ __launch_bounds__(kThreads) void residue_kernel(const int64_t *__restrict__ row_begin, const int64_t *__restrict__ row_count,
                                                           int max_rows, int64_t rows, const Slot *__restrict__ tables, int64_t cap,
                                                           int min_points, int64_t *out, int64_t out_stride) {
    const int b = blockIdx.y;
    int64_t begin;
    const int n = cloud_rows(row_begin, row_count, b, max_rows, rows, begin);
    if (n < 0) return;
    const int64_t used = pn2_slot_capacity(n);
    if ((int64_t)blockIdx.x * kThreads >= 2 * used) return;         // (uniform over the workgroup)
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    bool live = false;
    int64_t word = 0;                                               // class * 5 + (1: fp, a predicted segment; 2: fn, a ground-truth one)
    if (i < 2 * used) {
        const bool predicted = i >= used;
        const Slot s = tables[((int64_t)b * 3 + (predicted ? 1 : 0)) * cap + (predicted ? i - used : i)];
        if (s.key != kEmpty && s.matched == 0 && s.count >= min_points) {
            live = true;
            word = (int64_t)(s.key >> 32) * kColumns + (predicted ? 1 : 2);
        }
    }
    int64_t *dst = out + (int64_t)b * out_stride;
    if (kCombine) {
        const int lane = threadIdx.x & (PN2_WAVE - 1);
        live = pn2_wave_combine<kRounds>((long long)word, live, [&](bool, int leader, unsigned long long votes) {
            if (lane == leader) add_i64(dst + word, (unsigned long long)__popcll(votes));
        });
    }
    if (live) add_i64(dst + word, 1ull);
}

}  // namespace

extern "C" {

int64_t pn2_panoptic_workspace_bytes(int B, int64_t max_rows) {
    if (!pn2_slot_shape_ok(B, max_rows)) return PN2_EINVAL;
    return (int64_t)B * 3 * pn2_slot_capacity(max_rows) * (int64_t)sizeof(Slot);
}

int pn2_panoptic_count(const int32_t *pred_sem, const int32_t *pred_inst, const int32_t *gt_sem, const int32_t *gt_inst,
                       const int64_t *row_begin, const int64_t *row_count, int B, int64_t max_rows, int64_t rows, int C,
                       const int32_t *include, const int32_t *things, int min_points, int64_t *table, int64_t table_stride, int *err,
                       void *workspace, pn2_stream_t stream) {
    PN2_CHECK_ARG(pred_sem && pred_inst && gt_sem && gt_inst && row_begin && row_count && include && table && workspace);
    PN2_CHECK_ARG(pn2_slot_shape_ok(B, max_rows) && rows >= max_rows && C >= 1 && min_points >= 0);
    PN2_CHECK_ARG(table_stride == 0 || table_stride >= (int64_t)C * kColumns);
    PN2_CHECK_ARG(pn2_aligned(pred_sem, 4) && pn2_aligned(pred_inst, 4) && pn2_aligned(gt_sem, 4) && pn2_aligned(gt_inst, 4));
    PN2_CHECK_ARG(pn2_aligned(include, 4) && pn2_aligned(things, 4) && pn2_aligned(err, 4) && pn2_aligned(row_begin, 8) &&
                  pn2_aligned(row_count, 8) && pn2_aligned(table, 8) && pn2_aligned(workspace, 16));
    const int64_t cap = pn2_slot_capacity(max_rows);
    Slot *tables = static_cast<Slot *>(workspace);
    const hipStream_t s = pn2_s(stream);
    hipLaunchKernelGGL(clear_kernel, dim3(pn2_slot_clear_blocks(cap), (unsigned)B), dim3(kThreads), 0, s, row_begin, row_count, (int)max_rows, rows,
                       reinterpret_cast<uint4 *>(tables), cap);
    hipLaunchKernelGGL(count_kernel, dim3(pn2_slot_blocks(max_rows), (unsigned)B), dim3(kThreads), 0, s, pred_sem, pred_inst, gt_sem, gt_inst,
                       row_begin, row_count, (int)max_rows, rows, C, include, things, tables, cap, err);
    hipLaunchKernelGGL(match_kernel, dim3(pn2_slot_blocks(cap), (unsigned)B), dim3(kThreads), 0, s, row_begin, row_count, (int)max_rows, rows,
                       tables, cap, table, table_stride);
    hipLaunchKernelGGL(residue_kernel, dim3(pn2_slot_blocks(2 * cap), (unsigned)B), dim3(kThreads), 0, s, row_begin, row_count, (int)max_rows,
                       rows, tables, cap, min_points, table, table_stride);
    return pn2_launch_status();
}

}  // extern "C"
