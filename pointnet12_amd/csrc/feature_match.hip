// Feature matching: the two nearest candidate rows of every query row in feature space, and the filter that turns two such
// searches into a pair list: pn2_feature_nn2, pn2_match_pairs.  The rule is in include/pn2.h under "feature matching" and in numpy
// in tests/match_ref.py.
//
//   feature_nn2_kernel<W>   knn.hip's loop at a compile-time row width: ONE QUERY PER LANE, its row in W registers (D padded with
//                           zeros up to W: (0 - 0)^2 adds +0.0, the padded sum is the D-term sum bit for bit); the candidates are
//                           staged through LDS in tiles of kTileFloats / W rows and broadcast-read as float4; a candidate row that
//                           takes no part gets a NaN in column 0 (its distance is NaN and fails both compares), a query row that
//                           takes no part likewise.  Two (d2, j) slots per lane, strict compares, candidates in ascending j.
//                           A workgroup is 64 queries x 8 waves: every wave holds the same 64 query rows and takes every eighth
//                           row of a tile, and wave 0 merges the eight pairs of slots by ascending (d2, j) at the end -- the same
//                           two rows one scan would keep, and eight times the waves on a cloud of a few thousand rows.
//   match_rows_kernel       the clamped query count of every cloud as the int64 the compaction reads.
//   match_flag_kernel       compact.h's three passes as they stand: a flag per row (in range, mutual, ratio), the tile offsets,
//   match_write_kernel      the kept rows at their rank.  No atomics, nothing waits, the bytes are the same from run to run.
//
// This file is built with -ffp-contract=off: the distance is the separately rounded fp32 statement of the header.
#include <cmath>
#include "pn2_common.h"
#include "compact.h"

namespace {

constexpr int kQueries = PN2_WAVE;                                  // queries per workgroup: one per lane
constexpr int kSlices = 8;                                          // waves per workgroup: wave s takes rows s, s + 8, ... of every candidate tile
constexpr int kThreads = kQueries * kSlices;
constexpr int kTileFloats = 8192;                                   // 32 KiB of LDS: 128 rows at W = 64, 227 at W = 36

template <int W>
__global__ __launch_bounds__(kThreads) void feature_nn2_kernel(const float *__restrict__ query, int ldq, const float *__restrict__ cand, int ldc,
                                                               int N, int M, int D, const int64_t *__restrict__ n_query,
                                                               const int64_t *__restrict__ n_cand, int64_t *__restrict__ idx,
                                                               float *__restrict__ dist) {
    static_assert(W % 4 == 0, "rows are read as float4");
    constexpr int kRows = kTileFloats / W;
    __shared__ __attribute__((aligned(16))) float tile[kRows * W];
    __shared__ float s_d[kSlices][2][kQueries];
    __shared__ int s_j[kSlices][2][kQueries];
    const int b = blockIdx.y, t = threadIdx.x, lane = t & (PN2_WAVE - 1), slice = t / PN2_WAVE;
    const int nq = pn2_rows_or_all(n_query, b, N), mc = pn2_rows_or_all(n_cand, b, M);
    if ((int64_t)blockIdx.x * kQueries >= nq) return;               // (uniform over the workgroup)
    const int i = blockIdx.x * kQueries + lane;
    const bool live = i < nq;
    float q[W];
    {
        const float *row = query + ((int64_t)b * N + (live ? i : 0)) * ldq;
        bool finite = true, any = false;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            q[c] = c < D ? row[c] : 0.f;
            finite = finite && std::isfinite(q[c]);
            any = any || q[c] != 0.f;
        }
        if (!(finite && any)) q[0] = __builtin_nanf("");            // takes no part: every distance is NaN
    }
    float d0 = INFINITY, d1 = INFINITY;
    int j0 = M, j1 = M;
    const float *cb = cand + (int64_t)b * M * ldc;
    for (int base = 0; base < mc; base += kRows) {
        const int cnt = min(kRows, mc - base);
        __syncthreads();
        for (int e = t; e < cnt * W; e += kThreads) {
            const int k = e / W, c = e - k * W;
            tile[e] = c < D ? cb[(int64_t)(base + k) * ldc + c] : 0.f;
        }
        __syncthreads();
        for (int k = t; k < cnt; k += kThreads) {                   // (each lane its own rows, the columns rotated by the row: no bank is hit 64 times)
            bool finite = true, any = false;
            const int r = k % W;
#pragma unroll 4
            for (int c = 0; c < W; ++c) {
                int cc = c + r;
                cc -= cc >= W ? W : 0;
                const float v = tile[k * W + cc];
                finite = finite && std::isfinite(v);
                any = any || v != 0.f;
            }
            if (!(finite && any)) tile[k * W] = __builtin_nanf("");
        }
        __syncthreads();
        for (int k = slice; k < cnt; k += kSlices) {                // (ascending j inside a slice: strict compares keep the lower index)
            const float4 *row = reinterpret_cast<const float4 *>(tile + k * W);
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < W; c += 4) {
                const float4 f = row[c / 4];
                const float t0 = q[c] - f.x, t1 = q[c + 1] - f.y, t2 = q[c + 2] - f.z, t3 = q[c + 3] - f.w;
                s = s + t0 * t0;
                s = s + t1 * t1;
                s = s + t2 * t2;
                s = s + t3 * t3;
            }
            const int j = base + k;
            const bool lt0 = s < d0, lt1 = s < d1;                  // (NaN and +inf fail both)
            d1 = lt0 ? d0 : (lt1 ? s : d1);
            j1 = lt0 ? j0 : (lt1 ? j : j1);
            d0 = lt0 ? s : d0;
            j0 = lt0 ? j : j0;
        }
    }
    // the slices' best two meet through LDS; wave 0 merges them by ascending (d2, j): what one scan in ascending j would have kept
    s_d[slice][0][lane] = d0;
    s_d[slice][1][lane] = d1;
    s_j[slice][0][lane] = j0;
    s_j[slice][1][lane] = j1;
    __syncthreads();
    if (slice != 0 || !live) return;
#pragma unroll
    for (int w = 1; w < kSlices; ++w) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const float s = s_d[w][e][lane];
            const int j = s_j[w][e][lane];
            const bool lt0 = s < d0 || (s == d0 && j < j0), lt1 = s < d1 || (s == d1 && j < j1);          // ("none" is (+inf, M): never before anything)
            d1 = lt0 ? d0 : (lt1 ? s : d1);
            j1 = lt0 ? j0 : (lt1 ? j : j1);
            d0 = lt0 ? s : d0;
            j0 = lt0 ? j : j0;
        }
    }
    const int64_t o = ((int64_t)b * N + i) * 2;
    idx[o] = j0;
    idx[o + 1] = j1;
    dist[o] = d0;
    dist[o + 1] = d1;
}

__global__ __launch_bounds__(256) void match_rows_kernel(const int64_t *__restrict__ n_query, int B, int N, int64_t *__restrict__ rows) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) rows[b] = pn2_rows_or_all(n_query, b, N);
}

__global__ __launch_bounds__(kCompactThreads) void match_flag_kernel(const int64_t *__restrict__ idx, const float *__restrict__ dist,
                                                                     const int64_t *__restrict__ back, int N, int M, float ratio2,
                                                                     const int64_t *__restrict__ rows, unsigned char *__restrict__ flags,
                                                                     int *__restrict__ tile_count, int tiles) {
    const int b = blockIdx.y, tile = blockIdx.x;
    const int n = pn2_clamped_rows(rows, b, N);
    const int64_t t0 = (int64_t)tile * kCompactTile;
    if (t0 >= n) return;                                            // (uniform over the workgroup)
    const int64_t at = (int64_t)b * tiles + tile;
    const bool no_ratio = ratio2 == INFINITY;
    pn2_compact_flag_tile((int)(n - t0 < kCompactTile ? n - t0 : kCompactTile), flags + at * kCompactTile, tile_count + at, [&](int k) {
        const int64_t i = t0 + k, o = ((int64_t)b * N + i) * 2;
        const int64_t j = idx[o];
        if (j < 0 || j >= M) return false;
        if (back != nullptr && back[((int64_t)b * M + j) * 2] != i) return false;
        const float a = dist[o], c = dist[o + 1];
        return no_ratio || c == INFINITY || a <= ratio2 * c;
    });
}

__global__ __launch_bounds__(kCompactThreads) void match_write_kernel(const int64_t *__restrict__ idx, int N, const int64_t *__restrict__ rows,
                                                                      const unsigned char *__restrict__ flags, const int *__restrict__ tile_offset,
                                                                      int tiles, int64_t *__restrict__ pair_src, int64_t *__restrict__ pair_tgt) {
    const int b = blockIdx.y, tile = blockIdx.x;
    const int n = pn2_clamped_rows(rows, b, N);
    const int64_t t0 = (int64_t)tile * kCompactTile;
    if (t0 >= n) return;
    const int64_t at = (int64_t)b * tiles + tile;
    const int64_t out0 = (int64_t)b * N + tile_offset[at];
    pn2_compact_write_tile(flags + at * kCompactTile, [&](int k, int rank) {
        const int64_t i = t0 + k;
        pair_src[out0 + rank] = i;
        pair_tgt[out0 + rank] = idx[((int64_t)b * N + i) * 2];
    });
}

struct MatchWork {
    int64_t *rows;                  // [B]
    Pn2Compact compact;
    int64_t bytes;
};

MatchWork match_work(int B, int64_t N, void *base) {
    Pn2Arena a(base);
    return {a.take<int64_t>(B), pn2_compact_take(a, B, N), a.bytes()};
}

}  // namespace

extern "C" {

int pn2_feature_nn2(const float *query, int ldq, const float *cand, int ldc, int B, int N, int M, int D, const int64_t *n_query,
                    const int64_t *n_cand, int64_t *idx, float *dist, pn2_stream_t stream) {
    PN2_CHECK_ARG(query && cand && idx && dist);
    PN2_CHECK_ARG(pn2_cloud_shape_ok(B, N) && pn2_cloud_shape_ok(B, M) && D >= 1 && D <= ldq && D <= ldc);
    PN2_CHECK_ARG(pn2_aligned(query, 4) && pn2_aligned(cand, 4) && pn2_aligned(n_query, 8) && pn2_aligned(n_cand, 8) && pn2_aligned(idx, 8) &&
                  pn2_aligned(dist, 4));
    if (D > PN2_MATCH_MAX_D) return PN2_EUNSUPPORTED;
    const dim3 grid((unsigned)pn2_cdiv(N, kQueries), (unsigned)B);
    if (D <= 36)
        hipLaunchKernelGGL(feature_nn2_kernel<36>, grid, dim3(kThreads), 0, pn2_s(stream), query, ldq, cand, ldc, N, M, D, n_query, n_cand, idx, dist);
    else
        hipLaunchKernelGGL(feature_nn2_kernel<64>, grid, dim3(kThreads), 0, pn2_s(stream), query, ldq, cand, ldc, N, M, D, n_query, n_cand, idx, dist);
    return pn2_launch_status();
}

int64_t pn2_match_pairs_workspace_bytes(int B, int N) {
    if (!pn2_cloud_shape_ok(B, N)) return PN2_EINVAL;
    return match_work(B, N, nullptr).bytes;
}

int pn2_match_pairs(const int64_t *idx, const float *dist, const int64_t *back, int B, int N, int M, float ratio2, const int64_t *n_query,
                    int64_t *pair_src, int64_t *pair_tgt, int64_t *count, void *workspace, pn2_stream_t stream) {
    PN2_CHECK_ARG(idx && dist && pair_src && pair_tgt && count && workspace);
    PN2_CHECK_ARG(pn2_cloud_shape_ok(B, N) && pn2_cloud_shape_ok(B, M) && ratio2 >= 0.f);                  // (a NaN ratio2 fails the compare)
    PN2_CHECK_ARG(pn2_aligned(idx, 8) && pn2_aligned(dist, 4) && pn2_aligned(back, 8) && pn2_aligned(n_query, 8) && pn2_aligned(pair_src, 8) &&
                  pn2_aligned(pair_tgt, 8) && pn2_aligned(count, 8) && pn2_aligned(workspace, 16));
    const MatchWork w = match_work(B, N, workspace);
    const Pn2Compact &c = w.compact;
    const hipStream_t s = pn2_s(stream);
    const dim3 grid((unsigned)c.tiles, (unsigned)B);
    hipLaunchKernelGGL(match_rows_kernel, dim3((unsigned)pn2_cdiv(B, 256)), dim3(256), 0, s, n_query, B, N, w.rows);
    hipLaunchKernelGGL(match_flag_kernel, grid, dim3(kCompactThreads), 0, s, idx, dist, back, N, M, ratio2, w.rows, c.flags, c.tile_count,
                       c.tiles);
    hipLaunchKernelGGL(pn2_compact_offsets_kernel, dim3((unsigned)B), dim3(PN2_WAVE), 0, s, w.rows, N, c.tile_count, c.tile_offset, c.tiles,
                       count, (int *)nullptr, 0);
    hipLaunchKernelGGL(match_write_kernel, grid, dim3(kCompactThreads), 0, s, idx, N, w.rows, c.flags, c.tile_offset, c.tiles, pair_src,
                       pair_tgt);
    return pn2_launch_status();
}

}  // extern "C"
