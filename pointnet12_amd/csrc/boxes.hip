// Oriented bounding boxes per segment (include/pn2.h, "segment boxes"; in numpy: tests/box_ref.py): an L-shape fit swept over a
// caller-supplied table of angles.  For every segment of an `inverse`-style map and every angle a of the table the rows are projected
// on the angle's axes, the extent of the projections is taken, every row scores how close it lies to the nearest edge of that
// rectangle (the closeness criterion, quantised to an integer), and the angle with the largest score wins, the smaller area among
// equals, the lowest angle after that.
//
//   pn2_segment_boxes   six plain launches on the caller's stream, a launch boundary is the only ordering:
//     box_clear_kernel     the row counter of every segment and the cloud's list length to 0;
//     box_count_kernel     counts the rows of every segment that take part (integer atomicAdd, equal neighbours combined in the wave);
//     box_offsets_kernel   one wave per cloud: the exclusive prefix sum of the counts (the segments' buckets) and the list of the
//                          segments that hold at least `split_rows` rows;
//     box_scatter_kernel   every row that takes part writes its row number into its segment's bucket through an integer atomicAdd
//                          cursor;
//     box_sweep_kernel     a WAVE per segment below split_rows: lane L owns angle L of a block of 64 angles.  The wave loads 64
//                          bucket rows, one per lane, and walks them with a wave-uniform index (v_readlane: the row's x and y come
//                          out of the lanes' registers as scalars), so the walk has no memory access and no cross-lane reduction:
//                          each lane keeps the four extent keys of ITS angle, and in the second walk its int64 score.  A > 64: the
//                          block of 64 angles repeats.  A wave arg-best then picks the angle; lane 0 writes the row.  z and the raw
//                          box do not depend on the angle: each lane reduces its own rows once;
//     box_split_kernel     a WORKGROUP of 16 waves per listed segment: the waves share the bucket 64 rows at a time, combine their
//                          extent keys through LDS between the two walks and their scores after the second one.
//   THE ORDER INSIDE A BUCKET DIFFERS FROM RUN TO RUN (the cursor is an atomic), and which waves saw which rows differs between the two
//   sweep kernels.  Nothing that is written depends on either: an extent is a minimum or a maximum in a total order (the order-
//   preserving uint32 key of a float), a score is a sum of int32 terms in int64, n is a count, and u, v and a row's term are
//   functions of that row and the angle alone -- the second walk recomputes u and v with the very same operations.  So the bytes are
//   the same from run to run and whichever of the two kernels serves a segment.
//   No thread waits for another thread's write; no float atomics; no allocation; no host synchronisation.
//
// This file is built with -ffp-contract=off: every product, sum and difference of the rule is rounded on its own.
#include "wave_ops.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSweepWaves = kThreads / PN2_WAVE;                    // segments per workgroup of box_sweep_kernel
constexpr int kSplitWaves = 16;                                     // waves that share a listed segment
constexpr int kSplitDefault = 4096;                                 // split_rows = 0
constexpr float kMaxXY = 1152921504606846976.0f;                    // 2^60: the largest |x|, |y| that takes part

// the order-preserving key of a float32: -inf < ... < -0.0 < +0.0 < ... < +inf as unsigned integers
__device__ __forceinline__ unsigned key_of(float f) {
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float float_of(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
__device__ __forceinline__ unsigned umin(unsigned a, unsigned b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }
__device__ __forceinline__ float lane_value(float v, int j) {      // lane j's v, j uniform over the wave: a scalar
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}

struct Cols {
    int ld, cx, cy, cz;
};

struct Work {                                                       // the workspace: B * max_rows ints each, then B ints
    int *cnt, *cursor, *bucket, *list, *listed;
};
// (the struct goes to the kernels by value: the size comes back through `bytes`)
Work boxes_work(int B, int64_t max_rows, void *base, int64_t *bytes = nullptr) {
    Pn2Arena a(base);
    const int64_t n = (int64_t)B * max_rows;
    const Work w{a.take<int>(n), a.take<int>(n), a.take<int>(n), a.take<int>(n), a.take<int>(B)};
    if (bytes != nullptr) *bytes = a.bytes();
    return w;
}

struct Out {
    float *center, *size, *yaw, *lo, *hi;
    int32_t *angle, *n;
    long long *score;
};

// The segment row `i` of cloud b takes part in, -1 for none; `bits` collects the error bits.
__device__ __forceinline__ int row_segment(const float *__restrict__ pts, Cols col, const int32_t *__restrict__ seg, int64_t row, int m,
                                           int &bits) {
    const int s = seg[row];
    if (s < 0) return -1;
    if (s >= m) {                                                   // at or beyond out_count[b] (or max_rows)
        bits |= PN2_BOX_ERR_RANGE;
        return -1;
    }
    const float *p = pts + row * col.ld;
    const float x = p[col.cx], y = p[col.cy];
    const bool z_finite = (__float_as_uint(p[col.cz]) & 0x7F800000u) != 0x7F800000u;
    if (!(fabsf(x) <= kMaxXY && fabsf(y) <= kMaxXY && z_finite)) {  // (a NaN compares false)
        bits |= PN2_BOX_ERR_NONFINITE;
        return -1;
    }
    return s;
}

__device__ __forceinline__ void report(int *__restrict__ err, int bits) {
    const bool range = __any(bits & PN2_BOX_ERR_RANGE), nonfinite = __any(bits & PN2_BOX_ERR_NONFINITE);
    if (err != nullptr && (range || nonfinite) && (threadIdx.x & (PN2_WAVE - 1)) == 0)
        atomicOr(err, (range ? PN2_BOX_ERR_RANGE : 0) | (nonfinite ? PN2_BOX_ERR_NONFINITE : 0));
}

__global__ __launch_bounds__(kThreads) void box_clear_kernel(const int64_t *__restrict__ out_count, int max_rows, Work w) {
    const int b = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < pn2_clamped_rows(out_count, b, max_rows)) w.cnt[(int64_t)b * max_rows + i] = 0;
    if (i == 0) w.listed[b] = 0;
}

__global__ __launch_bounds__(kThreads) void box_count_kernel(const float *__restrict__ pts, Cols col, const int32_t *__restrict__ seg,
                                                             const int64_t *__restrict__ row_begin, const int64_t *__restrict__ row_count,
                                                             int max_rows, const int64_t *__restrict__ out_count, Work w,
                                                             int *__restrict__ err) {
    const int b = blockIdx.y;
    const int n = pn2_clamped_rows(row_count, b, max_rows), m = pn2_clamped_rows(out_count, b, max_rows);
    if ((int64_t)blockIdx.x * kThreads >= n) return;                // (uniform over the workgroup)
    const int i = blockIdx.x * kThreads + threadIdx.x, lane = threadIdx.x & (PN2_WAVE - 1);
    int bits = 0;
    const int s = i < n ? row_segment(pts, col, seg, row_begin[b] + i, m, bits) : -1;
    int *cnt = w.cnt + (int64_t)b * max_rows;
    // rows that follow each other mostly share a segment: the lanes of one segment add once
    const bool left = pn2_wave_combine<2>(s, s >= 0, [&](bool, int leader, unsigned long long votes) {
        if (lane == leader) atomicAdd(cnt + s, __popcll(votes));
    });
    if (left) atomicAdd(cnt + s, 1);
    report(err, bits);
}

// One wave per cloud: cursor[s] = cnt[0] + ... + cnt[s - 1], and the list of the segments with at least `split` rows.  The loop is
// pn2_wave_row_excl_scan's (wave_ops.h: 64 counts a step, a carry between) with the list built from the counts it already holds.
__global__ __launch_bounds__(PN2_WAVE) void box_offsets_kernel(const int64_t *__restrict__ out_count, int max_rows, int split, Work w) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int m = pn2_clamped_rows(out_count, b, max_rows);
    const int *cnt = w.cnt + (int64_t)b * max_rows;
    int *cursor = w.cursor + (int64_t)b * max_rows, *list = w.list + (int64_t)b * max_rows;
    int carry = 0, listed = 0;
    for (int first = 0; first < m; first += PN2_WAVE) {
        const int i = first + lane;
        const int v = i < m ? cnt[i] : 0;
        const int incl = pn2_wave_incl_scan(v);
        if (i < m) cursor[i] = carry + incl - v;
        carry += __shfl(incl, PN2_WAVE - 1, PN2_WAVE);
        const bool big = i < m && v >= split;
        const unsigned long long bigs = __ballot(big);
        if (big) list[listed + __popcll(bigs & ((1ull << lane) - 1ull))] = i;         // (at most m entries: in bounds)
        listed += __popcll(bigs);
    }
    if (lane == 0) w.listed[b] = listed;
}

__global__ __launch_bounds__(kThreads) void box_scatter_kernel(const float *__restrict__ pts, Cols col, const int32_t *__restrict__ seg,
                                                               const int64_t *__restrict__ row_begin, const int64_t *__restrict__ row_count,
                                                               int max_rows, const int64_t *__restrict__ out_count, Work w) {
    const int b = blockIdx.y;
    const int n = pn2_clamped_rows(row_count, b, max_rows), m = pn2_clamped_rows(out_count, b, max_rows);
    if ((int64_t)blockIdx.x * kThreads >= n) return;                // (uniform over the workgroup)
    const int i = blockIdx.x * kThreads + threadIdx.x, lane = threadIdx.x & (PN2_WAVE - 1);
    int bits = 0;
    const int s = i < n ? row_segment(pts, col, seg, row_begin[b] + i, m, bits) : -1;        // (the same decision as the count's)
    int *cursor = w.cursor + (int64_t)b * max_rows, *bucket = w.bucket + (int64_t)b * max_rows;
    const bool left = pn2_wave_combine<2>(s, s >= 0, [&](bool voter, int leader, unsigned long long votes) {
        int at = 0;
        if (lane == leader) at = atomicAdd(cursor + s, __popcll(votes));
        at = __shfl(at, leader, PN2_WAVE) + __popcll(votes & ((1ull << lane) - 1ull));
        if (voter && at < max_rows) bucket[at] = i;                 // (always: the buckets hold the rows that were counted, at most n)
    });
    if (left) {
        const int at = atomicAdd(cursor + s, 1);
        if (at < max_rows) bucket[at] = i;
    }
}

// ------------------------------------------------------------------------------------------------------------------ the sweep
struct Lds {                                                        // box_split_kernel's combines
    unsigned ext[kSplitWaves][PN2_WAVE][4];
    long long score[kSplitWaves][PN2_WAVE];
    unsigned box[kSplitWaves][6];
};

// The box of ONE segment whose rows are bucket[begin .. end), by W waves (1, or the kSplitWaves waves of a workgroup: every wave
// of it calls this with the same arguments).  `o` is the output row.
template <int W>
__device__ __forceinline__ void sweep_segment(const float *__restrict__ pts, Cols col, int64_t row0, int n, const int *__restrict__ bucket,
                                              int begin, int end, const float4 *__restrict__ table, int A, float d0, Out out, int64_t o,
                                              Lds *lds) {
    const int lane = threadIdx.x & (PN2_WAVE - 1), wave = W == 1 ? 0 : (int)(threadIdx.x / PN2_WAVE);
    const bool writer = lane == 0 && wave == 0;
    if (begin >= end) {                                             // (uniform over the W waves) a segment without rows
        if (writer) {
            for (int c = 0; c < 3; ++c) {
                out.center[o * 3 + c] = 0.0f;
                out.size[o * 3 + c] = 0.0f;
                if (out.lo != nullptr) out.lo[o * 3 + c] = 0.0f;
                if (out.hi != nullptr) out.hi[o * 3 + c] = 0.0f;
            }
            out.yaw[o] = 0.0f;
            if (out.angle != nullptr) out.angle[o] = -1;
            if (out.n != nullptr) out.n[o] = 0;
            if (out.score != nullptr) out.score[o] = 0;
        }
        return;
    }
    // the row a lane holds of the 64 rows from bucket position k on (a row number outside the cloud cannot happen; it is never addressed)
    auto row_of = [&](int k) -> const float * {
        const int at = k + lane;
        if (at >= end) return nullptr;
        const int r = bucket[at];
        return (unsigned)r < (unsigned)n ? pts + (row0 + r) * col.ld : nullptr;
    };

    // z and the raw box: every lane reduces the rows it holds, the wave (and the workgroup) combines six keys
    unsigned lo[3] = {~0u, ~0u, ~0u}, hi[3] = {0u, 0u, 0u};
    for (int k = begin + wave * PN2_WAVE; k < end; k += W * PN2_WAVE) {
        const float *p = row_of(k);
        if (p != nullptr) {
            const unsigned kx = key_of(p[col.cx]), ky = key_of(p[col.cy]), kz = key_of(p[col.cz]);
            lo[0] = umin(lo[0], kx), hi[0] = umax(hi[0], kx);
            lo[1] = umin(lo[1], ky), hi[1] = umax(hi[1], ky);
            lo[2] = umin(lo[2], kz), hi[2] = umax(hi[2], kz);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            lo[c] = umin(lo[c], (unsigned)__shfl_xor((int)lo[c], d, PN2_WAVE));
            hi[c] = umax(hi[c], (unsigned)__shfl_xor((int)hi[c], d, PN2_WAVE));
        }
    }
    if (W > 1) {
        if (lane == 0)
            for (int c = 0; c < 3; ++c) lds->box[wave][c] = lo[c], lds->box[wave][3 + c] = hi[c];
        __syncthreads();
#pragma nounroll
        for (int w = 0; w < W; ++w)
            for (int c = 0; c < 3; ++c) lo[c] = umin(lo[c], lds->box[w][c]), hi[c] = umax(hi[c], lds->box[w][3 + c]);
    }

    long long best_score = -1;                                      // what the angles visited so far chose (the same on every lane)
    float best_area = 0.0f, best_c = 1.0f, best_s = 0.0f, best_yaw = 0.0f, bu0 = 0.0f, bu1 = 0.0f, bv0 = 0.0f, bv1 = 0.0f;
    int best_a = -1;
    for (int first = 0; first < A; first += PN2_WAVE) {
        const int a = first + lane;
        const bool valid = a < A;
        const float4 t = valid ? table[a] : make_float4(1.0f, 0.0f, 0.0f, 0.0f);
        float c = t.x, s = t.y, yaw = t.z;
        PN2_OPAQUE3(c, s, yaw);                                     // (plain 32-bit values, no register tuple: pn2_common.h, PN2_OPAQUE)
        // first walk: the extent of this lane's angle
        unsigned ku0 = ~0u, ku1 = 0u, kv0 = ~0u, kv1 = 0u;
        for (int k = begin + wave * PN2_WAVE; k < end; k += W * PN2_WAVE) {
            const float *p = row_of(k);
            const bool held = p != nullptr;
            const float x = held ? p[col.cx] : 0.0f, y = held ? p[col.cy] : 0.0f;
            const unsigned long long rows = __ballot(held);
            const int cnt = end - k < PN2_WAVE ? end - k : PN2_WAVE;
            for (int j = 0; j < cnt; ++j) {
                if (!((rows >> j) & 1ull)) continue;                // (uniform; cannot happen)
                const float xj = lane_value(x, j), yj = lane_value(y, j);
                const float u = (c * xj) + (s * yj), v = (c * yj) - (s * xj);
                const unsigned ku = key_of(u), kv = key_of(v);
                ku0 = umin(ku0, ku), ku1 = umax(ku1, ku);
                kv0 = umin(kv0, kv), kv1 = umax(kv1, kv);
            }
        }
        if (W > 1) {
            __syncthreads();                                        // (the box keys, or the block before this one, have been read)
            lds->ext[wave][lane][0] = ku0, lds->ext[wave][lane][1] = ku1, lds->ext[wave][lane][2] = kv0, lds->ext[wave][lane][3] = kv1;
            __syncthreads();
#pragma nounroll
            for (int w = 0; w < W; ++w) {
                ku0 = umin(ku0, lds->ext[w][lane][0]), ku1 = umax(ku1, lds->ext[w][lane][1]);
                kv0 = umin(kv0, lds->ext[w][lane][2]), kv1 = umax(kv1, lds->ext[w][lane][3]);
            }
        }
        const float u0 = float_of(ku0), u1 = float_of(ku1), v0 = float_of(kv0), v1 = float_of(kv1);
        // second walk: the closeness score of this lane's angle (u and v by the same operations as above)
        long long score = 0;
        if (d0 > 0.0f) {
            for (int k = begin + wave * PN2_WAVE; k < end; k += W * PN2_WAVE) {
                const float *p = row_of(k);
                const bool held = p != nullptr;
                const float x = held ? p[col.cx] : 0.0f, y = held ? p[col.cy] : 0.0f;
                const unsigned long long rows = __ballot(held);
                const int cnt = end - k < PN2_WAVE ? end - k : PN2_WAVE;
                for (int j = 0; j < cnt; ++j) {
                    if (!((rows >> j) & 1ull)) continue;
                    const float xj = lane_value(x, j), yj = lane_value(y, j);
                    const float u = (c * xj) + (s * yj), v = (c * yj) - (s * xj);
                    const float e = fminf(fminf(u - u0, u1 - u), fminf(v - v0, v1 - v));
                    const float d = fmaxf(e, d0);
                    const float q = d0 / d;                         // one IEEE float32 division
                    score += (int)(q * 1048576.0f);                 // exact product, truncated: 0 .. 2^20
                }
            }
            if (W > 1) {
                lds->score[wave][lane] = score;
                __syncthreads();
                score = 0;
#pragma nounroll
                for (int w = 0; w < W; ++w) score += lds->score[w][lane];
            }
        }
        const float lu = u1 - u0, lv = v1 - v0;
        const float area = lu * lv;
        // the block's best angle: the largest score, the smaller area among equals, the lowest angle after that
        long long ws = valid ? score : -1;
        float wa = area;
        int wi = a;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const long long os = __shfl_xor(ws, d, PN2_WAVE);
            const float oa = __shfl_xor(wa, d, PN2_WAVE);
            const int oi = __shfl_xor(wi, d, PN2_WAVE);
            if (os > ws || (os == ws && (oa < wa || (oa == wa && oi < wi)))) ws = os, wa = oa, wi = oi;
        }
        if (ws > best_score || (ws == best_score && wa < best_area)) {        // (uniform) a strict improvement on the blocks before
            const int from = wi - first;
            best_score = ws, best_area = wa, best_a = wi;
            best_c = __shfl(c, from, PN2_WAVE), best_s = __shfl(s, from, PN2_WAVE), best_yaw = __shfl(yaw, from, PN2_WAVE);
            bu0 = __shfl(u0, from, PN2_WAVE), bu1 = __shfl(u1, from, PN2_WAVE);
            bv0 = __shfl(v0, from, PN2_WAVE), bv1 = __shfl(v1, from, PN2_WAVE);
        }
    }
    if (!writer) return;
    const float z0 = float_of(lo[2]), z1 = float_of(hi[2]);
    float cu = 0.5f * (bu0 + bu1), cv = 0.5f * (bv0 + bv1);
    // The four products one after the other, each one's operands held back until the product before it exists: the compiler would
    // pack them two by two with a register pair read through its high half (pn2_common.h, PN2_OPAQUE; tools/check_isa.py pkhi).
    const float cxu = best_c * cu;
    asm volatile("" : "+v"(best_s), "+v"(cv) : "v"(cxu));
    const float sxv = best_s * cv;
    asm volatile("" : "+v"(best_s), "+v"(cu) : "v"(sxv));
    const float sxu = best_s * cu;
    asm volatile("" : "+v"(best_c), "+v"(cv) : "v"(sxu));
    const float cxv = best_c * cv;
    out.center[o * 3 + 0] = cxu - sxv;
    out.center[o * 3 + 1] = sxu + cxv;
    out.center[o * 3 + 2] = 0.5f * (z0 + z1);
    out.size[o * 3 + 0] = bu1 - bu0;
    out.size[o * 3 + 1] = bv1 - bv0;
    out.size[o * 3 + 2] = z1 - z0;
    out.yaw[o] = best_yaw;
    if (out.angle != nullptr) out.angle[o] = best_a;
    for (int c = 0; c < 3; ++c) {
        if (out.lo != nullptr) out.lo[o * 3 + c] = float_of(lo[c]);
        if (out.hi != nullptr) out.hi[o * 3 + c] = float_of(hi[c]);
    }
    if (out.n != nullptr) out.n[o] = end - begin;
    if (out.score != nullptr) out.score[o] = best_score;
}

__global__ __launch_bounds__(kThreads) void box_sweep_kernel(const float *__restrict__ pts, Cols col, const int64_t *__restrict__ row_begin,
                                                             const int64_t *__restrict__ row_count, int max_rows,
                                                             const int64_t *__restrict__ out_begin, const int64_t *__restrict__ out_count,
                                                             const float4 *__restrict__ table, int A, float d0, int split, Work w, Out out) {
    const int b = blockIdx.y;
    const int m = pn2_clamped_rows(out_count, b, max_rows);
    const int64_t s = (int64_t)blockIdx.x * kSweepWaves + threadIdx.x / PN2_WAVE;
    if (s >= m) return;                                             // (uniform over the wave; no barrier below)
    const int64_t base = (int64_t)b * max_rows;
    const int cnt = w.cnt[base + s];
    if (cnt >= split) return;                                       // box_split_kernel's
    const int end = w.cursor[base + s], begin = end - cnt;          // (the scatter moved the cursor to the bucket's end)
    if (cnt < 0 || begin < 0 || end > max_rows) return;             // (cannot happen)
    sweep_segment<1>(pts, col, row_begin[b], pn2_clamped_rows(row_count, b, max_rows), w.bucket + base, begin, end, table, A, d0, out,
                     out_begin[b] + s, nullptr);
}

__global__ __launch_bounds__(kSplitWaves *PN2_WAVE) void box_split_kernel(const float *__restrict__ pts, Cols col,
                                                                           const int64_t *__restrict__ row_begin,
                                                                           const int64_t *__restrict__ row_count, int max_rows,
                                                                           const int64_t *__restrict__ out_begin,
                                                                           const int64_t *__restrict__ out_count,
                                                                           const float4 *__restrict__ table, int A, float d0, Work w, Out out) {
    __shared__ Lds lds;
    const int b = blockIdx.y;
    if ((int)blockIdx.x >= w.listed[b]) return;                     // (uniform over the workgroup)
    const int64_t base = (int64_t)b * max_rows;
    const int s = w.list[base + blockIdx.x];
    if (s < 0 || s >= pn2_clamped_rows(out_count, b, max_rows)) return;      // (cannot happen)
    const int cnt = w.cnt[base + s], end = w.cursor[base + s], begin = end - cnt;
    if (cnt <= 0 || begin < 0 || end > max_rows) return;            // (cannot happen)
    sweep_segment<kSplitWaves>(pts, col, row_begin[b], pn2_clamped_rows(row_count, b, max_rows), w.bucket + base, begin, end, table, A, d0,
                               out, out_begin[b] + s, &lds);
}

inline bool shape_ok(int B, int64_t max_rows) { return B >= 1 && B <= 65535 && max_rows >= 0 && max_rows <= PN2_VOXEL_MAX_ROWS; }

}  // namespace

extern "C" {

int64_t pn2_segment_boxes_workspace_bytes(int B, int64_t max_rows) {
    int64_t bytes = PN2_EINVAL;
    if (shape_ok(B, max_rows)) boxes_work(B, max_rows, nullptr, &bytes);
    return bytes;
}

int pn2_segment_boxes(const float *pts, int ld, int cx, int cy, int cz, const int32_t *seg, const int64_t *row_begin, const int64_t *row_count,
                      int B, int64_t max_rows, const int64_t *out_begin, const int64_t *out_count, const float *angles, int A, float d0,
                      int split_rows, float *center, float *size, float *yaw, int32_t *angle, float *lo, float *hi, int32_t *n,
                      int64_t *score, int *err, void *workspace, pn2_stream_t stream) {
    PN2_CHECK_ARG(pts && seg && row_begin && row_count && out_begin && out_count && angles && center && size && yaw && workspace);
    PN2_CHECK_ARG(shape_ok(B, max_rows) && A >= 1 && A <= PN2_BOX_MAX_ANGLES && ld >= 1);
    PN2_CHECK_ARG(cx >= 0 && cy >= 0 && cz >= 0 && cx < ld && cy < ld && cz < ld && cx != cy && cx != cz && cy != cz);
    PN2_CHECK_ARG(d0 == d0 && d0 - d0 == 0.0f);                     // finite
    PN2_CHECK_ARG(split_rows == 0 || (split_rows >= PN2_WAVE && split_rows <= PN2_VOXEL_MAX_ROWS));
    PN2_CHECK_ARG(pn2_aligned(pts, 4) && pn2_aligned(seg, 4) && pn2_aligned(angles, 16) && pn2_aligned(center, 4) && pn2_aligned(size, 4) &&
                  pn2_aligned(yaw, 4) && pn2_aligned(angle, 4) && pn2_aligned(lo, 4) && pn2_aligned(hi, 4) && pn2_aligned(n, 4) &&
                  pn2_aligned(score, 8) && pn2_aligned(err, 4) && pn2_aligned(workspace, 16));
    const int split = split_rows == 0 ? kSplitDefault : split_rows;
    const Work w = boxes_work(B, max_rows, workspace);
    const Cols col{ld, cx, cy, cz};
    const Out out{center, size, yaw, lo, hi, angle, n, reinterpret_cast<long long *>(score)};
    const float4 *table = reinterpret_cast<const float4 *>(angles);
    const hipStream_t s = pn2_s(stream);
    const int R = (int)max_rows;
    const auto blocks = [](int64_t items, int64_t per) { return (unsigned)(items <= 0 ? 1 : pn2_cdiv(items, per)); };
    const dim3 by_row(blocks(max_rows, kThreads), (unsigned)B);
    hipLaunchKernelGGL(box_clear_kernel, by_row, dim3(kThreads), 0, s, out_count, R, w);
    hipLaunchKernelGGL(box_count_kernel, by_row, dim3(kThreads), 0, s, pts, col, seg, row_begin, row_count, R, out_count, w, err);
    hipLaunchKernelGGL(box_offsets_kernel, dim3((unsigned)B), dim3(PN2_WAVE), 0, s, out_count, R, split, w);
    hipLaunchKernelGGL(box_scatter_kernel, by_row, dim3(kThreads), 0, s, pts, col, seg, row_begin, row_count, R, out_count, w);
    hipLaunchKernelGGL(box_sweep_kernel, dim3(blocks(max_rows, kSweepWaves), (unsigned)B), dim3(kThreads), 0, s, pts, col, row_begin, row_count, R,
                       out_begin, out_count, table, A, d0, split, w, out);
    // at most max_rows / split segments of a cloud reach the list
    hipLaunchKernelGGL(box_split_kernel, dim3(blocks(max_rows / split, 1), (unsigned)B), dim3(kSplitWaves * PN2_WAVE), 0, s, pts, col, row_begin,
                       row_count, R, out_begin, out_count, table, A, d0, w, out);
    return pn2_launch_status();
}

}  // extern "C"
