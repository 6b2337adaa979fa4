// K nearest neighbours for general K (1 <= K <= 32) and the majority vote over them: pn2_knn, pn2_knn_vote (include/pn2.h).
//
// COMPILED WITH -ffp-contract=off: the distance is pair_dist of pair_dist.h, the arithmetic of pn2_three_nn and
// pn2_square_distance, bit for bit.
#include "pn2_common.h"
#include "pair_dist.h"

namespace {

constexpr int KNN_TILE = 1024;
constexpr int KNN_THREADS = 256;

// ---------------------------------------------------------------------------------------------
// One query per lane; the candidates are staged through LDS as (x, y, z, |p|^2) tiles and broadcast-read, as
// three_nn_kernel does.  Each lane keeps its CAP best (d2, index) pairs in registers, ascending; a candidate is tested
// against the worst of them first (strict <), and only then walks the compare-and-shift chain -- fully unrolled over the
// compile-time capacity, so every array index is a constant and nothing goes to scratch.  Candidates arrive in ascending
// index and every compare is strict: equal distances keep their index order, i.e. the first K of a stable sort.  A NaN or
// +inf distance fails every compare and is never kept.  The lane holds the CAP best and writes the first K of them.
// ---------------------------------------------------------------------------------------------
template <int CAP>
__global__ __launch_bounds__(KNN_THREADS) void knn_kernel(const float *__restrict__ query, const float *__restrict__ cand, int N,
                                                          int M, int K, const int64_t *__restrict__ n_query,
                                                          const int64_t *__restrict__ n_cand, int64_t *__restrict__ idx,
                                                          float *__restrict__ dist) {
    __shared__ float4 tile[KNN_TILE];
    const int b = blockIdx.y;
    const int nq_b = pn2_rows_or_all(n_query, b, N), mc = pn2_rows_or_all(n_cand, b, M);
    if ((int)(blockIdx.x * KNN_THREADS) >= nq_b) return;                  // (block-uniform: no barrier is skipped by a part of it)
    const int n = blockIdx.x * KNN_THREADS + threadIdx.x;
    const bool live = n < nq_b;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (live) {
        const float *q = query + ((size_t)b * N + n) * 3;
        qx = q[0]; qy = q[1]; qz = q[2];
    }
    const float nq = sq_norm3(qx, qy, qz);
    float bd[CAP];
    int bi[CAP];
#pragma unroll
    for (int s = 0; s < CAP; ++s) { bd[s] = INFINITY; bi[s] = M; }
    const float *c = cand + (size_t)b * M * 3;
    for (int base = 0; base < mc; base += KNN_TILE) {
        const int cnt = min(KNN_TILE, mc - base);
        __syncthreads();
        for (int k = threadIdx.x; k < cnt; k += KNN_THREADS) {
            const float x = c[3 * (size_t)(base + k)], y = c[3 * (size_t)(base + k) + 1], z = c[3 * (size_t)(base + k) + 2];
            tile[k] = make_float4(x, y, z, sq_norm3(x, y, z));
        }
        __syncthreads();
        if (live) {
            for (int k = 0; k < cnt; ++k) {
                const float4 v = tile[k];
                const float d = pair_dist(qx, qy, qz, nq, v.x, v.y, v.z, v.w);
                if (d < bd[CAP - 1]) {
                    const int j = base + k;
                    bool lt[CAP];
#pragma unroll
                    for (int s = 0; s < CAP; ++s) lt[s] = d < bd[s];
#pragma unroll
                    for (int s = CAP - 1; s > 0; --s) {               // slot s: the old slot s-1 moves down, or d lands here, or it stays
                        bd[s] = lt[s - 1] ? bd[s - 1] : (lt[s] ? d : bd[s]);
                        bi[s] = lt[s - 1] ? bi[s - 1] : (lt[s] ? j : bi[s]);
                    }
                    bd[0] = lt[0] ? d : bd[0];
                    bi[0] = lt[0] ? j : bi[0];
                }
            }
        }
    }
    if (!live) return;
    const size_t o = ((size_t)b * N + n) * K;
#pragma unroll
    for (int s = 0; s < CAP; ++s) {
        if (s < K) {
            idx[o + s] = bi[s];
            if (dist != nullptr) dist[o + s] = bd[s];
        }
    }
}

template <int CAP>
int launch_knn(const float *query, const float *cand, int B, int N, int M, int K, const int64_t *n_query, const int64_t *n_cand,
               int64_t *idx, float *dist, hipStream_t s) {
    hipLaunchKernelGGL(knn_kernel<CAP>, dim3((unsigned)pn2_cdiv(N, KNN_THREADS), B), dim3(KNN_THREADS), 0, s, query, cand, N, M, K,
                       n_query, n_cand, idx, dist);
    return pn2_launch_status();
}

// ---------------------------------------------------------------------------------------------
// Majority vote: one row per lane, its K slots in registers.  The count of a slot's label is the number of voting slots
// that carry the same label -- slots are compared with one another (each pair once, CAP (CAP - 1) / 2 compares, unrolled),
// so there is no per-class histogram, no class limit and no runtime-indexed array.  Scanning the slots in ascending order
// with a strict > leaves the label whose first voting slot comes first among those with the largest count.  Integers only.
// ---------------------------------------------------------------------------------------------
template <int CAP>
__global__ __launch_bounds__(256) void knn_vote_kernel(const int64_t *__restrict__ idx, const float *__restrict__ dist,
                                                       const int64_t *__restrict__ cand_label, int N, int M, int K, float max_d2,
                                                       const int64_t *__restrict__ n_query, int32_t fill,
                                                       const int32_t *__restrict__ lut, int L, const int32_t *__restrict__ dst,
                                                       int64_t out_stride, int32_t *__restrict__ out, int32_t *__restrict__ err) {
    const int b = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= pn2_rows_or_all(n_query, b, N)) return;
    const size_t o = ((size_t)b * N + n) * K;
    const int64_t *labels = cand_label + (size_t)b * M;
    int64_t lab[CAP];
    bool votes[CAP];
    int cnt[CAP];
#pragma unroll
    for (int s = 0; s < CAP; ++s) {
        votes[s] = false;
        lab[s] = 0;
        if (s < K) {
            const int64_t i = idx[o + s];
            const float d = dist[o + s];
            votes[s] = i >= 0 && i < M && !(d > max_d2);
            if (votes[s]) lab[s] = labels[i];
        }
        cnt[s] = votes[s] ? 1 : 0;
    }
#pragma unroll
    for (int s = 1; s < CAP; ++s) {
#pragma unroll
        for (int t = 0; t < s; ++t) {
            const int same = (votes[s] && votes[t] && lab[s] == lab[t]) ? 1 : 0;
            cnt[s] += same;
            cnt[t] += same;
        }
    }
    int best = 0;
    int64_t win = 0;
#pragma unroll
    for (int s = 0; s < CAP; ++s) {
        const bool take = cnt[s] > best;
        best = take ? cnt[s] : best;
        win = take ? lab[s] : win;
    }
    int flags = 0;
    int32_t res = fill;
    if (best > 0) {
        if (lut != nullptr) {
            if (win >= 0 && win < L) res = lut[win];
            else flags |= 1;
        } else {
            res = (int32_t)win;
        }
    }
    int64_t pos = n;
    bool write = true;
    if (dst != nullptr) {
        pos = dst[(size_t)b * N + n];
        if (pos < 0 || pos >= out_stride) { write = false; flags |= 2; }
    }
    if (write) out[(size_t)b * out_stride + pos] = res;
    if (flags != 0 && err != nullptr) atomicOr(err, flags);
}

template <int CAP>
int launch_knn_vote(const int64_t *idx, const float *dist, const int64_t *cand_label, int B, int N, int M, int K, float max_d2,
                    const int64_t *n_query, int32_t fill, const int32_t *lut, int L, const int32_t *dst, int64_t out_stride,
                    int32_t *out, int32_t *err, hipStream_t s) {
    hipLaunchKernelGGL(knn_vote_kernel<CAP>, dim3((unsigned)pn2_cdiv(N, 256), B), dim3(256), 0, s, idx, dist, cand_label, N, M, K,
                       max_d2, n_query, fill, lut, L, dst, out_stride, out, err);
    return pn2_launch_status();
}

}  // namespace

extern "C" {

int pn2_knn(const float *query, const float *cand, int B, int N, int M, int K, const int64_t *n_query, const int64_t *n_cand,
            int64_t *idx, float *dist, pn2_stream_t stream) {
    PN2_CHECK_ARG(query && cand && idx && B > 0 && N > 0 && M > 0 && K >= 1 && B <= 65535 && N <= 0x7FFFFF00);
    if (K > 32) return PN2_EUNSUPPORTED;
    PN2_CHECK_ARG(K <= M);
    hipStream_t s = pn2_s(stream);
    if (K <= 4) return launch_knn<4>(query, cand, B, N, M, K, n_query, n_cand, idx, dist, s);
    if (K <= 8) return launch_knn<8>(query, cand, B, N, M, K, n_query, n_cand, idx, dist, s);
    if (K <= 16) return launch_knn<16>(query, cand, B, N, M, K, n_query, n_cand, idx, dist, s);
    return launch_knn<32>(query, cand, B, N, M, K, n_query, n_cand, idx, dist, s);
}

int pn2_knn_vote(const int64_t *idx, const float *dist, const int64_t *cand_label, int B, int N, int M, int K, float max_d2,
                 const int64_t *n_query, int32_t fill, const int32_t *lut, int L, const int32_t *dst, int64_t out_stride,
                 int32_t *out, int32_t *err, pn2_stream_t stream) {
    PN2_CHECK_ARG(idx && dist && cand_label && out && B > 0 && N > 0 && M > 0 && K >= 1 && B <= 65535 && N <= 0x7FFFFF00);
    PN2_CHECK_ARG(out_stride > 0 && (dst != nullptr || out_stride >= N) && (lut == nullptr || L > 0));
    if (K > 32) return PN2_EUNSUPPORTED;
    hipStream_t s = pn2_s(stream);
    if (K <= 4) return launch_knn_vote<4>(idx, dist, cand_label, B, N, M, K, max_d2, n_query, fill, lut, L, dst, out_stride, out, err, s);
    if (K <= 8) return launch_knn_vote<8>(idx, dist, cand_label, B, N, M, K, max_d2, n_query, fill, lut, L, dst, out_stride, out, err, s);
    if (K <= 16) return launch_knn_vote<16>(idx, dist, cand_label, B, N, M, K, max_d2, n_query, fill, lut, L, dst, out_stride, out, err, s);
    return launch_knn_vote<32>(idx, dist, cand_label, B, N, M, K, max_d2, n_query, fill, lut, L, dst, out_stride, out, err, s);
}

}  // extern "C"
