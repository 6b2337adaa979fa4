// Order-free segment reductions over an `inverse`-style map (include/pn2.h, "segment reductions"): the MEAN of every segment's rows,
// its backward pass, and the MAJORITY LABEL -- the voxel centroid and the voxel label of pn2_voxel_grid's cells, and a pooling layer
// for anything else that comes with such a map.  Everything that crosses threads is an INTEGER atomic (max, add, compare-and-swap):
// integer maxima and sums commute, so nothing that is written out depends on arrival order, hash layout, wave aggregation or grid
// shape, and the result is the same from run to run, byte for byte, with no sort and no fixed-order sum.
//
//   pn2_segment_mean   four plain launches on the caller's stream, a launch boundary is the only ordering:
//     mean_clear_kernel     K (int32), S (int64) of every (segment, column) and the row counter of every segment to 0;
//     mean_max_kernel       K = integer atomicMax of the terms' exponents k (255: a NaN / inf term); counts the rows unless the caller
//                           brought n_points;
//     mean_add_kernel       S += t, a 64-bit integer atomicAdd of the fixed-point term t = +-((M << 10) >> (K - k));
//     mean_final_kernel     one thread per (segment, column): float32(ldexp(double(S) / double(n), K - 160)).
//   Lane L of a wave holds column L % C of row L / C of the wave's 64 / C rows, so one wave instruction touches adjacent words of a
//   segment's accumulator row (option SEGRED_LANES = 0: one row per lane, its columns in a loop); rows of a scan that follow each
//   other mostly share a cell, so runs of equal segment are combined inside the wave (a segmented suffix reduction over shuffles,
//   skipped by a wave that holds no run) and only a run's first row issues the atomic (option SEGRED_COMBINE; integer addition is
//   associative: the bytes are the same either way).  64-bit integer atomics at these shapes are unmeasured in the hardware notes
//   this project follows (their prices are for float atomics): tools/bench_voxel_reduce.py times every form (README: the table).
//   pn2_segment_mean_bwd  one gather-and-divide launch.
//   pn2_segment_mode   four launches: the open-addressing table of slot_table.h with the key (rank << 32 | label) and atomicAdd of
//     the pair's count (runs of equal pairs are added once per wave run), used at the capacity of the cloud's device-side row
//     count; then every occupied slot does a 64-bit atomicMax on its segment's winner word (count << 32 | 0x7FFFFFFF - label:
//     most votes, then the LOWEST label), and a last launch decodes it.
//   No thread waits for another thread's write.
//
// This file is built with -ffp-contract=off: the division and the power-of-two scaling are separately rounded operations.
#include <cmath>
#include "slot_table.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / PN2_WAVE;
constexpr int kNonFinite = 255;
constexpr unsigned kQuietNan = 0x7FC00000u;

struct alignas(16) Pair {
    unsigned long long key;                                         // rank << 32 | label
    int votes;
    int unused;
};
static_assert(sizeof(Pair) == 16, "one slot is one 16-byte word");
static_assert(kThreads == kSlotThreads, "mode_clear_kernel fills its table with pn2_slot_fill; the grids come from pn2_slot_blocks");

// ----------------------------------------------------------------------------------------------------------------- the mean
// What a lane of the two row passes works on: row i of cloud b (column c), its segment (-1: the lane takes no part) and, for the
// run combining, whether its row starts a run of equal segments inside the wave and the lane that stands for that run.
struct Term {
    int64_t row;                                                    // the row in `values`
    int seg;
    int c, cstep;                                                   // the lane's columns: c, c + cstep, ... below C (the same count on every lane)
    int step;                                                       // lanes between two rows of the wave: C, or 1 with a row per lane
    int run;                                                        // first lane of the run's first row (unique per lane when idle)
    bool head, bad;
    unsigned long long heads0, rows0;                               // ballots over each row's first lane: run starts, rows in use
};

__device__ __forceinline__ bool load_term(Term &t, const int32_t *__restrict__ seg, const int64_t *__restrict__ row_begin,
                                          const int64_t *__restrict__ row_count, int max_rows, const int64_t *__restrict__ out_count,
                                          int C, int R, bool by_row) {
    const int b = blockIdx.y;
    const int n = pn2_clamped_rows(row_count, b, max_rows), m = pn2_clamped_rows(out_count, b, max_rows);
    const int64_t first = (int64_t)blockIdx.x * (kWaves * R);
    if (first >= n) return false;                                   // (uniform over the workgroup)
    const int lane = threadIdx.x & (PN2_WAVE - 1), wave = threadIdx.x / PN2_WAVE;
    const int r = by_row ? lane : lane / C;
    t.c = by_row ? 0 : lane - r * C;
    t.cstep = t.step = by_row ? 1 : C;
    const bool used = r < R;
    const int64_t i = first + (int64_t)wave * R + r;
    t.seg = -1;
    t.bad = false;
    t.row = 0;
    if (used && i < n) {
        t.row = row_begin[b] + i;
        const int s = seg[t.row];
        if (s >= m) t.bad = true;                                   // at or beyond out_count[b] (or max_rows): takes no part
        else if (s >= 0) t.seg = s;
    }
    const int before = __shfl_up(t.seg, t.step, PN2_WAVE);
    t.head = r == 0 || before != t.seg;
    t.heads0 = __ballot(used && t.c == 0 && t.head);
    t.rows0 = __ballot(used && t.c == 0);
    // the nearest run start at or before this lane's row (bit 0 is always set: row 0 starts a run)
    const unsigned long long upto = t.heads0 & (lane == 63 ? ~0ull : (2ull << lane) - 1ull);
    t.run = used ? 63 - __clzll((long long)upto) : PN2_WAVE + lane;
    return true;
}

// rows of the run that starts at this lane (a row's first lane, a run's first row)
__device__ __forceinline__ int run_rows(const Term &t, int lane) {
    const unsigned long long later = lane == 63 ? 0ull : t.heads0 >> (lane + 1);
    const int next = later ? lane + __ffsll((long long)later) : PN2_WAVE;          // the next run's lane, or the end of the wave
    const unsigned long long below_next = next >= PN2_WAVE ? ~0ull : (1ull << next) - 1ull;
    return __popcll(t.rows0 & below_next & ~((1ull << lane) - 1ull));
}

template <bool kCombine>
__global__ __launch_bounds__(kThreads) void mean_max_kernel(const float *__restrict__ values, int ld, int C, int R,
                                                            const int32_t *__restrict__ seg, const int64_t *__restrict__ row_begin,
                                                            const int64_t *__restrict__ row_count, int max_rows,
                                                            const int64_t *__restrict__ out_count, int *__restrict__ K,
                                                            int *__restrict__ rows_of, int *__restrict__ err, bool by_row) {
    Term t;
    if (!load_term(t, seg, row_begin, row_count, max_rows, out_count, C, R, by_row)) return;
    const int lane = threadIdx.x & (PN2_WAVE - 1);
    const bool runs = kCombine && t.heads0 != t.rows0;              // (uniform over the wave) some row continues its predecessor's segment
    const bool issue = t.seg >= 0 && (!kCombine || t.head);
    const int rows = kCombine ? run_rows(t, lane) : 1;
    const int64_t word = (int64_t)blockIdx.y * max_rows + t.seg;
    for (int c = t.c; c < C; c += t.cstep) {
        int k = 0;
        if (t.seg >= 0) {
            const unsigned bits = reinterpret_cast<const unsigned *>(values)[t.row * ld + c];
            const int e = (int)((bits >> 23) & 255u);
            k = e == 255 ? kNonFinite : (e == 0 ? 1 : e);
        }
        if (runs) {
            for (int d = t.step; d < R * t.step; d <<= 1) {         // segmented suffix maximum: after the step a lane holds 2 d / step rows of its run
                const int other = __shfl_down(k, d, PN2_WAVE), its = __shfl_down(t.run, d, PN2_WAVE);
                if (lane + d < PN2_WAVE && its == t.run) k = other > k ? other : k;
            }
        }
        if (issue) {
            atomicMax(K + word * C + c, k);
            if (rows_of != nullptr && c == 0) atomicAdd(rows_of + word, rows);
        }
    }
    if (err != nullptr && __any(t.bad) && lane == 0) atomicOr(err, PN2_SEGMENT_ERR_RANGE);
}

template <bool kCombine>
__global__ __launch_bounds__(kThreads) void mean_add_kernel(const float *__restrict__ values, int ld, int C, int R,
                                                            const int32_t *__restrict__ seg, const int64_t *__restrict__ row_begin,
                                                            const int64_t *__restrict__ row_count, int max_rows,
                                                            const int64_t *__restrict__ out_count, const int *__restrict__ K,
                                                            long long *__restrict__ S, bool by_row) {
    Term t;
    if (!load_term(t, seg, row_begin, row_count, max_rows, out_count, C, R, by_row)) return;
    const int lane = threadIdx.x & (PN2_WAVE - 1);
    const bool runs = kCombine && t.heads0 != t.rows0;              // (uniform over the wave)
    const bool issue = t.seg >= 0 && (!kCombine || t.head);
    for (int c = t.c; c < C; c += t.cstep) {
        long long term = 0;
        int64_t word = 0;
        if (t.seg >= 0) {
            word = ((int64_t)blockIdx.y * max_rows + t.seg) * C + c;
            const int top = K[word];                                // (the launch before this one wrote it)
            if (top != kNonFinite) {
                const unsigned bits = reinterpret_cast<const unsigned *>(values)[t.row * ld + c];
                const int e = (int)((bits >> 23) & 255u);
                const unsigned long long M = e == 0 ? (bits & 0x7FFFFFu) : ((bits & 0x7FFFFFu) | 0x800000u);
                const unsigned down = (unsigned)(top - (e == 0 ? 1 : e));
                const long long mag = down >= 34u ? 0ll : (long long)((M << 10) >> down);   // the shift truncates the magnitude
                term = (bits >> 31) ? -mag : mag;
            }
        }
        if (runs) {
            for (int d = t.step; d < R * t.step; d <<= 1) {         // segmented suffix sum over the run (at most 64 terms below 2^34)
                const long long other = __shfl_down(term, d, PN2_WAVE);
                const int its = __shfl_down(t.run, d, PN2_WAVE);
                if (lane + d < PN2_WAVE && its == t.run) term += other;
            }
        }
        if (issue && term != 0) atomicAdd(reinterpret_cast<unsigned long long *>(S + word), (unsigned long long)term);
    }
}

__global__ __launch_bounds__(kThreads) void mean_clear_kernel(const int64_t *__restrict__ out_count, int max_rows, int C,
                                                              int *__restrict__ K, long long *__restrict__ S, int *__restrict__ rows_of) {
    const int b = blockIdx.y;
    const int64_t words = (int64_t)pn2_clamped_rows(out_count, b, max_rows) * C;
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= words) return;
    const int64_t at = (int64_t)b * max_rows * C + e;
    K[at] = 0;
    S[at] = 0;
    if (e % C == 0) rows_of[(int64_t)b * max_rows + e / C] = 0;
}

__global__ __launch_bounds__(kThreads) void mean_final_kernel(const int64_t *__restrict__ out_begin, const int64_t *__restrict__ out_count,
                                                              int max_rows, int C, const int *__restrict__ K,
                                                              const long long *__restrict__ S, const int *__restrict__ rows_of,
                                                              const int32_t *__restrict__ n_points, float *__restrict__ out, int ld_out,
                                                              int32_t *__restrict__ n_out, int *__restrict__ err) {
    const int b = blockIdx.y;
    const int64_t words = (int64_t)pn2_clamped_rows(out_count, b, max_rows) * C;
    if ((int64_t)blockIdx.x * kThreads >= words) return;            // (uniform over the workgroup)
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    bool nonfinite = false;
    if (e < words) {
        const int64_t s = e / C;
        const int c = (int)(e - s * C);
        const int64_t o = out_begin[b] + s;
        const int n = n_points != nullptr ? n_points[o] : rows_of[(int64_t)b * max_rows + s];
        const int64_t at = (int64_t)b * max_rows * C + e;
        const int top = K[at];
        unsigned bits = 0u;                                         // a segment without rows: +0.0
        if (top == kNonFinite) {
            bits = kQuietNan;
            nonfinite = true;
        } else if (n > 0 && top > 0) {
            const double q = (double)S[at] / (double)n;             // int64 -> fp64 to nearest even, one IEEE division
            bits = __float_as_uint((float)ldexp(q, top - 160));     // an exact scaling, then ONE rounding to float32
        }
        reinterpret_cast<unsigned *>(out)[o * ld_out + c] = bits;
        if (n_out != nullptr && c == 0) n_out[o] = n;
    }
    if (err != nullptr && __any(nonfinite) && (threadIdx.x & (PN2_WAVE - 1)) == 0) atomicOr(err, PN2_SEGMENT_ERR_NONFINITE);
}

__global__ __launch_bounds__(kThreads) void mean_bwd_kernel(const float *__restrict__ grad_out, int ld_out, int C,
                                                            const int32_t *__restrict__ seg, const int64_t *__restrict__ row_begin,
                                                            const int64_t *__restrict__ row_count, int max_rows,
                                                            const int64_t *__restrict__ out_begin, const int64_t *__restrict__ out_count,
                                                            const int32_t *__restrict__ n_points, float *__restrict__ grad_in, int ld_in,
                                                            int *__restrict__ err) {
    const int b = blockIdx.y;
    const int64_t words = (int64_t)pn2_clamped_rows(row_count, b, max_rows) * C;
    if ((int64_t)blockIdx.x * kThreads >= words) return;            // (uniform over the workgroup)
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    bool bad = false;
    if (e < words) {
        const int m = pn2_clamped_rows(out_count, b, max_rows);
        const int64_t i = e / C;
        const int c = (int)(e - i * C);
        const int64_t row = row_begin[b] + i;
        const int s = seg[row];
        float g = 0.0f;                                             // a row that takes no part
        if (s >= m) {
            bad = true;
        } else if (s >= 0) {
            const int64_t o = out_begin[b] + s;
            const int n = n_points[o];
            if (n > 0) g = grad_out[o * ld_out + c] / (float)n;     // one IEEE float32 division
        }
        grad_in[row * ld_in + c] = g;
    }
    if (err != nullptr && __any(bad) && (threadIdx.x & (PN2_WAVE - 1)) == 0) atomicOr(err, PN2_SEGMENT_ERR_RANGE);
}

// ----------------------------------------------------------------------------------------------------------------- the mode
__global__ __launch_bounds__(kThreads) void mode_clear_kernel(const int64_t *__restrict__ row_count, const int64_t *__restrict__ out_count,
                                                              int max_rows, uint4 *__restrict__ table, int64_t cap,
                                                              unsigned long long *__restrict__ winner) {
    const int b = blockIdx.y;
    pn2_slot_fill(table + (int64_t)b * cap, pn2_slot_capacity(pn2_clamped_rows(row_count, b, max_rows)), pn2_slot_empty(0u, 0u));     // the slots in USE: <= cap
    const int64_t m = pn2_clamped_rows(out_count, b, max_rows);
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < m; i += (int64_t)gridDim.x * kThreads)
        winner[(int64_t)b * max_rows + i] = 0ull;
}

template <bool kCombine>
__global__ __launch_bounds__(kThreads) void mode_insert_kernel(const int32_t *__restrict__ labels, const int32_t *__restrict__ seg,
                                                               const int64_t *__restrict__ row_begin,
                                                               const int64_t *__restrict__ row_count, int max_rows,
                                                               const int64_t *__restrict__ out_count, Pair *__restrict__ table, int64_t cap,
                                                               int *__restrict__ err) {
    const int b = blockIdx.y;
    const int n = pn2_clamped_rows(row_count, b, max_rows);
    if ((int64_t)blockIdx.x * kThreads >= n) return;                // (uniform over the workgroup)
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & (PN2_WAVE - 1);
    unsigned long long key = kEmpty;                                // no vote
    bool bad = false;
    if (i < n) {
        const int m = pn2_clamped_rows(out_count, b, max_rows);
        const int64_t row = row_begin[b] + i;
        const int s = seg[row];
        if (s >= m) {
            bad = true;
        } else if (s >= 0) {
            const int label = labels[row];
            if (label >= 0) key = ((unsigned long long)(unsigned)s << 32) | (unsigned)label;
        }
    }
    int votes = 1;
    bool issue = key != kEmpty;
    if (kCombine) {                                                 // a run of equal (segment, label) pairs votes once, with its length
        const unsigned long long before = __shfl_up(key, 1, PN2_WAVE);
        const bool head = lane == 0 || before != key;
        const unsigned long long heads = __ballot(head);
        const unsigned long long later = lane == 63 ? 0ull : heads >> (lane + 1);
        votes = later ? __ffsll((long long)later) : PN2_WAVE - lane;
        issue = issue && head;
    }
    if (issue) {
        Pair *tab = table + (int64_t)b * cap;
        const int slot = pn2_slot_claim(tab, (unsigned)pn2_slot_capacity(n) - 1u, key);
        if (slot >= 0) atomicAdd(&tab[slot].votes, votes);          // (always: the cloud has at most half as many rows as slots)
    }
    if (err != nullptr && __any(bad) && lane == 0) atomicOr(err, PN2_SEGMENT_ERR_RANGE);
}

__global__ __launch_bounds__(kThreads) void mode_vote_kernel(const int64_t *__restrict__ row_count, const int64_t *__restrict__ out_count,
                                                             int max_rows, const Pair *__restrict__ table, int64_t cap,
                                                             unsigned long long *__restrict__ winner) {
    const int b = blockIdx.y;
    const int64_t slots = pn2_slot_capacity(pn2_clamped_rows(row_count, b, max_rows));
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= slots) return;
    const Pair p = table[(int64_t)b * cap + i];
    if (p.key == kEmpty) return;
    const unsigned rank = (unsigned)(p.key >> 32), label = (unsigned)p.key;
    if ((int)rank >= pn2_clamped_rows(out_count, b, max_rows)) return;       // (cannot happen: the insert checked it)
    // most votes first, then the LOWEST label: the word is never 0, a vote count is at least 1
    atomicMax(winner + (int64_t)b * max_rows + rank, ((unsigned long long)(unsigned)p.votes << 32) | (0x7FFFFFFFu - label));
}

__global__ __launch_bounds__(kThreads) void mode_decode_kernel(const int64_t *__restrict__ out_begin, const int64_t *__restrict__ out_count,
                                                               int max_rows, const unsigned long long *__restrict__ winner, int32_t fill,
                                                               int32_t *__restrict__ out_labels, int32_t *__restrict__ votes) {
    const int b = blockIdx.y;
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= pn2_clamped_rows(out_count, b, max_rows)) return;
    const unsigned long long w = winner[(int64_t)b * max_rows + s];
    const int64_t o = out_begin[b] + s;
    if (out_labels != nullptr) out_labels[o] = w == 0ull ? fill : (int32_t)(0x7FFFFFFFu - (unsigned)w);
    if (votes != nullptr) votes[o] = (int32_t)(w >> 32);
}

// the workspace of the mean: a sum and a maximum per (segment, column), a row count per segment
struct MeanWork {
    long long *S;
    int *K, *rows_of;
    int64_t bytes;
};
MeanWork mean_work(int B, int64_t max_rows, int C, void *base) {
    Pn2Arena a(base);
    const int64_t n = (int64_t)B * max_rows;
    return {a.take<long long>(n * C), a.take<int>(n * C), a.take<int>(n), a.bytes()};
}

// the workspace of the mode: the (segment, label) tables, a winner word per segment
struct ModeWork {
    Pair *table;
    unsigned long long *winner;
    int64_t cap, bytes;                                             // cap: slots of one cloud's table
};
ModeWork mode_work(int B, int64_t max_rows, void *base) {
    Pn2Arena a(base);
    const int64_t cap = pn2_slot_capacity(max_rows);
    return {a.take<Pair>(B * cap), a.take<unsigned long long>((int64_t)B * max_rows), cap, a.bytes()};
}

}  // namespace

extern "C" {

int64_t pn2_segment_reduce_workspace_bytes(int B, int64_t max_rows, int C) {
    if (!pn2_slot_shape_ok(B, max_rows) || C < 1 || C > PN2_SEGMENT_MAX_COLS) return PN2_EINVAL;
    const int64_t mean = mean_work(B, max_rows, C, nullptr).bytes, mode = mode_work(B, max_rows, nullptr).bytes;
    return mean > mode ? mean : mode;
}

int pn2_segment_mean(const float *values, int ld, int C, const int32_t *seg, const int64_t *row_begin, const int64_t *row_count, int B,
                     int64_t max_rows, const int64_t *out_begin, const int64_t *out_count, const int32_t *n_points, float *out, int ld_out,
                     int32_t *n_out, int *err, void *workspace, pn2_stream_t stream) {
    PN2_CHECK_ARG(values && seg && row_begin && row_count && out_begin && out_count && out && workspace);
    PN2_CHECK_ARG(pn2_slot_shape_ok(B, max_rows) && C >= 1 && C <= PN2_SEGMENT_MAX_COLS && ld >= C && ld_out >= C);
    PN2_CHECK_ARG(pn2_aligned(values, 4) && pn2_aligned(out, 4) && pn2_aligned(seg, 4) && pn2_aligned(workspace, 16));
    const MeanWork w = mean_work(B, max_rows, C, workspace);
    const bool row_per_lane = pn2_opt(PN2_OPT_SEGRED_LANES) == 0;   // (A/B: one row per lane, its columns in a loop)
    const int R = row_per_lane ? PN2_WAVE : PN2_WAVE / C;           // rows per wave of the two row passes
    const hipStream_t s = pn2_s(stream);
    const dim3 by_word(pn2_slot_blocks(max_rows * C), (unsigned)B), by_row(pn2_slot_blocks(pn2_cdiv(max_rows, kWaves * R) * kThreads), (unsigned)B);
    int *count_here = n_points == nullptr ? w.rows_of : nullptr;
    hipLaunchKernelGGL(mean_clear_kernel, by_word, dim3(kThreads), 0, s, out_count, (int)max_rows, C, w.K, w.S, w.rows_of);
    if (pn2_opt(PN2_OPT_SEGRED_COMBINE)) {
        hipLaunchKernelGGL(mean_max_kernel<true>, by_row, dim3(kThreads), 0, s, values, ld, C, R, seg, row_begin, row_count, (int)max_rows,
                           out_count, w.K, count_here, err, row_per_lane);
        hipLaunchKernelGGL(mean_add_kernel<true>, by_row, dim3(kThreads), 0, s, values, ld, C, R, seg, row_begin, row_count, (int)max_rows,
                           out_count, w.K, w.S, row_per_lane);
    } else {
        hipLaunchKernelGGL(mean_max_kernel<false>, by_row, dim3(kThreads), 0, s, values, ld, C, R, seg, row_begin, row_count, (int)max_rows,
                           out_count, w.K, count_here, err, row_per_lane);
        hipLaunchKernelGGL(mean_add_kernel<false>, by_row, dim3(kThreads), 0, s, values, ld, C, R, seg, row_begin, row_count, (int)max_rows,
                           out_count, w.K, w.S, row_per_lane);
    }
    hipLaunchKernelGGL(mean_final_kernel, by_word, dim3(kThreads), 0, s, out_begin, out_count, (int)max_rows, C, w.K, w.S, w.rows_of, n_points, out,
                       ld_out, n_out, err);
    return pn2_launch_status();
}

int pn2_segment_mean_bwd(const float *grad_out, int ld_out, int C, const int32_t *seg, const int64_t *row_begin, const int64_t *row_count,
                         int B, int64_t max_rows, const int64_t *out_begin, const int64_t *out_count, const int32_t *n_points,
                         float *grad_in, int ld_in, int *err, pn2_stream_t stream) {
    PN2_CHECK_ARG(grad_out && seg && row_begin && row_count && out_begin && out_count && n_points && grad_in);
    PN2_CHECK_ARG(pn2_slot_shape_ok(B, max_rows) && C >= 1 && C <= PN2_SEGMENT_MAX_COLS && ld_out >= C && ld_in >= C);
    PN2_CHECK_ARG(pn2_aligned(grad_out, 4) && pn2_aligned(grad_in, 4) && pn2_aligned(seg, 4) && pn2_aligned(n_points, 4));
    hipLaunchKernelGGL(mean_bwd_kernel, dim3(pn2_slot_blocks(max_rows * C), (unsigned)B), dim3(kThreads), 0, pn2_s(stream), grad_out, ld_out, C,
                       seg, row_begin, row_count, (int)max_rows, out_begin, out_count, n_points, grad_in, ld_in, err);
    return pn2_launch_status();
}

int pn2_segment_mode(const int32_t *labels, const int32_t *seg, const int64_t *row_begin, const int64_t *row_count, int B, int64_t max_rows,
                     const int64_t *out_begin, const int64_t *out_count, int32_t fill, int32_t *out_labels, int32_t *votes, int *err,
                     void *workspace, pn2_stream_t stream) {
    PN2_CHECK_ARG(labels && seg && row_begin && row_count && out_begin && out_count && workspace && (out_labels || votes));
    PN2_CHECK_ARG(pn2_slot_shape_ok(B, max_rows) && pn2_aligned(labels, 4) && pn2_aligned(seg, 4) && pn2_aligned(workspace, 16));
    const ModeWork w = mode_work(B, max_rows, workspace);
    const int64_t cap = w.cap;
    const hipStream_t s = pn2_s(stream);
    const dim3 by_row(pn2_slot_blocks(max_rows), (unsigned)B);
    hipLaunchKernelGGL(mode_clear_kernel, dim3(pn2_slot_clear_blocks(cap), (unsigned)B), dim3(kThreads), 0, s, row_count, out_count, (int)max_rows,
                       reinterpret_cast<uint4 *>(w.table), cap, w.winner);
    if (pn2_opt(PN2_OPT_SEGRED_COMBINE))
        hipLaunchKernelGGL(mode_insert_kernel<true>, by_row, dim3(kThreads), 0, s, labels, seg, row_begin, row_count, (int)max_rows,
                           out_count, w.table, cap, err);
    else
        hipLaunchKernelGGL(mode_insert_kernel<false>, by_row, dim3(kThreads), 0, s, labels, seg, row_begin, row_count, (int)max_rows,
                           out_count, w.table, cap, err);
    hipLaunchKernelGGL(mode_vote_kernel, dim3(pn2_slot_blocks(cap), (unsigned)B), dim3(kThreads), 0, s, row_count, out_count, (int)max_rows, w.table,
                       cap, w.winner);
    hipLaunchKernelGGL(mode_decode_kernel, by_row, dim3(kThreads), 0, s, out_begin, out_count, (int)max_rows, w.winner, fill, out_labels, votes);
    return pn2_launch_status();
}

}  // extern "C"
