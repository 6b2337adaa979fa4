// Chamfer distance (reference model/chamfer.py): for every query point of p1 the nearest candidate of p2, as an all-pairs
// search that never writes anything of size N x M.
//     value = (1/B) sum_b sum_n min_m || p1[b,n,:] - p2[b,m,:] ||_2        (one direction, the distance and not its square)
// The reference repeats both sets to [B,N,M,D], subtracts, takes the norm and a min over M.  Here a thread keeps QPT query
// points in registers, the candidates pass through LDS in tiles and every lane reads the SAME candidate (a broadcast
// ds_read_b128 feeds QPT distance evaluations), the running (d^2, index) pair lives in registers.
//
// Numerics (they are the contract, include/pn2.h):
//   * d^2 in DIFFERENCE form, fp32: t_0 = q_0 - c_0, d2 = t_0 * t_0, then d2 = fmaf(t_k, t_k, d2) for k = 1 .. D-1 in index
//     order.  Not the |a|^2 + |b|^2 - 2ab expansion of three_nn_kernel: its absolute error of ~1e-7 |p|^2 in d^2 turns into
//     ~3e-4 |p| in d for near-coincident points once the square root is taken.
//   * strict `<` over candidates in ascending index: ties (on that fp32 d^2) go to the LOWEST index; the same rule joins the
//     partial results when the candidates of a cloud are split over workgroups (ascending ranges, strict `<`).
//   * one correctly rounded square root per query, after the search: sqrtf, which hipcc rounds correctly by default; without
//     OCML_BASIC_ROUNDED_OPERATIONS __fsqrt_rn is v_sqrt_f32 alone, which is one ulp off on some values.
//   * the scalar is summed in a fixed order: fp64 per-workgroup partials (a fixed shuffle tree), then ONE workgroup adds the
//     partials in index order -- dist, idx and the value are bit-identical from run to run.
#include "pn2_common.h"

#include <algorithm>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxD = 16;
constexpr int kMaxSplits = 64;       // candidate ranges per cloud, at most
constexpr int kMinChunk = 128;       // candidates per range, at least (and ranges are multiples of it)

template <int D>
struct TileShape {
    static constexpr int DP = (D + 3) & ~3;                              // LDS row pitch in floats: rows are read as float4
    static constexpr int CT = DP <= 4 ? 1024 : DP <= 8 ? 512 : 256;      // candidates per tile: 16 KiB of LDS
};

// How one call is cut into workgroups.  A workgroup owns 256 * qpt queries of one cloud and one contiguous range of `chunk`
// candidates.  With few queries (a single cloud of a few thousand points) the grid would cover a handful of the CUs: then
// one query per thread and the candidates split into up to kMaxSplits ranges, joined by chamfer_join_kernel.
struct Plan {
    int qpt, qtiles, splits, chunk;
    int64_t partials;                // fp64 partial sums the finishing kernel writes
};

Plan make_plan(int B, int N, int M) {
    Plan p;
    const int64_t target = 2 * (int64_t)pn2_num_cus();
    const int max_splits = (int)std::min<int64_t>(kMaxSplits, pn2_cdiv(M, kMinChunk));
    p.qpt = 4;
    if ((int64_t)B * pn2_cdiv(N, kThreads * 4) * max_splits < target) p.qpt = 1;
    p.qtiles = (int)pn2_cdiv(N, kThreads * p.qpt);
    const int64_t wgs = (int64_t)B * p.qtiles;
    int want = (int)std::min<int64_t>(max_splits, pn2_cdiv(target, wgs));
    if (want < 1) want = 1;
    p.chunk = (int)(pn2_cdiv(pn2_cdiv(M, want), kMinChunk) * kMinChunk);
    p.splits = (int)pn2_cdiv(M, p.chunk);                               // every range is non-empty
    p.partials = p.splits == 1 ? wgs : pn2_cdiv((int64_t)B * N, kThreads);
    return p;
}

// The workspace: the fp64 partials (rounded to 256 bytes); with split candidates each query's best pair per range, the distances
// then the indices back to back.
struct Work {
    double *partials;
    float *part_d2;
    int *part_idx;
    int64_t bytes;
};
Work chamfer_work(const Plan &p, int B, int N, void *base) {
    Pn2Arena a(base);
    const int64_t pairs = p.splits > 1 ? (int64_t)B * N * p.splits : 0;        // (nothing taken, both null, without a join)
    return {a.take<double>(p.partials, 256), pairs ? a.take<float>(pairs, 4) : nullptr, pairs ? a.take<int>(pairs, 4) : nullptr, a.bytes()};
}

// Sum of `v` over the workgroup in a fixed shape (xor-shuffle tree, then the four waves in order); valid in thread 0.
__device__ __forceinline__ double block_sum_f64(double v) {
    __shared__ double sh[kThreads / 64];
    v = pn2_wave_sum_f64(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < kThreads / 64; ++i) s += sh[i];
    return s;
}

// grid (query tiles, candidate ranges, B).  splits == 1: writes dist / idx and the workgroup's partial sum; otherwise the
// range's (d^2, index) per query into part_d2 / part_idx [B*N, splits].
template <int D, int QPT>
__global__ __launch_bounds__(kThreads) void chamfer_nn_kernel(const float *__restrict__ p1, const float *__restrict__ p2, int N,
                                                              int M, int chunk, int splits, float *__restrict__ dist,
                                                              int64_t *__restrict__ idx, float *__restrict__ part_d2,
                                                              int *__restrict__ part_idx, double *__restrict__ partials) {
    constexpr int DP = TileShape<D>::DP, CT = TileShape<D>::CT, Q4 = DP / 4;
    __shared__ float4 tile[CT * Q4];
    float *tile_f = reinterpret_cast<float *>(tile);
    const int b = blockIdx.z, s = blockIdx.y;
    const int n0 = blockIdx.x * (kThreads * QPT) + threadIdx.x;       // this thread's queries: n0 + i * 256

    float q[QPT][D];
    float best[QPT];
    int arg[QPT];
#pragma unroll
    for (int i = 0; i < QPT; ++i) {
        const int n = n0 + i * kThreads;
        const float *src = p1 + ((size_t)b * N + (n < N ? n : 0)) * D;      // (a dead query searches for point 0; nothing is stored)
#pragma unroll
        for (int d = 0; d < D; ++d) q[i][d] = src[d];
        best[i] = INFINITY;
        arg[i] = 0;
    }

    const int m0 = s * chunk, m1 = min(M, m0 + chunk);
    const float *cand = p2 + (size_t)b * M * D;
    for (int base = m0; base < m1; base += CT) {
        const int cnt = min(CT, m1 - base);
        __syncthreads();                                                  // the previous tile has been read by every wave
        const float *src = cand + (size_t)base * D;
        for (int e = threadIdx.x; e < cnt * D; e += kThreads) {           // contiguous in memory; rows re-pitched to DP in LDS
            const int r = e / D, c = e - r * D;
            tile_f[r * DP + c] = src[e];
        }
        __syncthreads();
        auto visit = [&](int k) {                                         // candidate base + k against the QPT queries
            float v[DP];
#pragma unroll
            for (int j = 0; j < Q4; ++j) {
                const float4 t = tile[k * Q4 + j];
                v[4 * j] = t.x; v[4 * j + 1] = t.y; v[4 * j + 2] = t.z; v[4 * j + 3] = t.w;
            }
#pragma unroll
            for (int d = 0; d < D; ++d) PN2_OPAQUE1(v[d]);                // no packed op may select the high half of the LDS tuple
#pragma unroll
            for (int i = 0; i < QPT; ++i) {
                const float t0 = q[i][0] - v[0];
                float d2 = t0 * t0;
#pragma unroll
                for (int d = 1; d < D; ++d) {
                    const float t = q[i][d] - v[d];
                    d2 = fmaf(t, t, d2);
                }
                if (d2 < best[i]) { best[i] = d2; arg[i] = base + k; }
            }
        };
        int k = 0;
        for (; k + 4 <= cnt; k += 4) {                                    // (unrolled by hand: `#pragma unroll 4` is refused here)
#pragma unroll
            for (int u = 0; u < 4; ++u) visit(k + u);
        }
        for (; k < cnt; ++k) visit(k);
    }

    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < QPT; ++i) {
        const int n = n0 + i * kThreads;
        if (n >= N) continue;
        const size_t o = (size_t)b * N + n;
        if (splits == 1) {
            const float dd = sqrtf(best[i]);                              // (not __fsqrt_rn: that is the 1-ulp native root here)
            dist[o] = dd;
            idx[o] = arg[i];
            acc += (double)dd;
        } else {
            part_d2[o * splits + s] = best[i];
            part_idx[o * splits + s] = arg[i];
        }
    }
    if (splits == 1 && partials != nullptr) {
        const double total = block_sum_f64(acc);
        if (threadIdx.x == 0) partials[(size_t)blockIdx.z * gridDim.x + blockIdx.x] = total;
    }
}

// Joins the candidate ranges of a query in ascending order with the same strict `<`: on equal d^2 the lower range, that is
// the lower index, stays.  One thread per query.
__global__ __launch_bounds__(kThreads) void chamfer_join_kernel(const float *__restrict__ part_d2, const int *__restrict__ part_idx,
                                                                int64_t total, int splits, float *__restrict__ dist,
                                                                int64_t *__restrict__ idx, double *__restrict__ partials) {
    const int64_t o = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    double acc = 0.0;
    if (o < total) {
        float best = INFINITY;
        int arg = 0;
        for (int s = 0; s < splits; ++s) {
            const float d2 = part_d2[o * splits + s];
            if (d2 < best) { best = d2; arg = part_idx[o * splits + s]; }
        }
        const float dd = sqrtf(best);
        dist[o] = dd;
        idx[o] = arg;
        acc = (double)dd;
    }
    if (partials != nullptr) {
        const double sum = block_sum_f64(acc);
        if (threadIdx.x == 0) partials[blockIdx.x] = sum;
    }
}

// One workgroup: thread t adds partials t, t + 256, ... in index order, then a fixed tree -- the order is a function of the
// partial count only.  *out = sum / B.
__global__ __launch_bounds__(kThreads) void chamfer_sum_kernel(const double *__restrict__ partials, int64_t count, int B,
                                                               float *__restrict__ out) {
    __shared__ double tree[kThreads];
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < count; i += kThreads) v += partials[i];
    tree[threadIdx.x] = v;
    __syncthreads();
    for (int w = kThreads / 2; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) tree[threadIdx.x] += tree[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = (float)tree[0] / (float)B;           // the reference: an fp32 sum divided by B
}

// One thread per (query, component).  dp1 = (g / B) (p1 - p2[idx]) / dist, a zero row where dist == 0 (the backward of
// torch.norm at the origin); dp2[idx] -= the same (fp32 atomics: dp2 is accumulated, the caller zeroes it).
__global__ __launch_bounds__(kThreads) void chamfer_bwd_kernel(const float *__restrict__ p1, const float *__restrict__ p2,
                                                               const float *__restrict__ dist, const int64_t *__restrict__ idx,
                                                               const float *__restrict__ g, int B, int N, int M, int D,
                                                               int64_t total, float *__restrict__ dp1, float *__restrict__ dp2) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= total) return;
    const int64_t o = e / D;                  // b * N + n
    const int c = (int)(e - o * D);
    const int64_t b = o / N;
    const float d = dist[o];
    const int64_t j = idx[o];
    float v = 0.f;
    const bool hit = d > 0.f && j >= 0 && j < M;
    const int64_t t = hit ? (b * M + j) * D + c : 0;
    if (hit) {
        const float scale = __fdiv_rn(*g, (float)B);
        v = __fdiv_rn(p1[e] - p2[t], d) * scale;
    }
    if (dp1 != nullptr) dp1[e] = v;
    if (dp2 != nullptr && v != 0.f) atomicAdd(dp2 + t, -v);
}

template <int D, int QPT>
void launch_nn(const Plan &p, const float *p1, const float *p2, int B, int N, int M, float *dist, int64_t *idx, float *part_d2,
               int *part_idx, double *partials, hipStream_t s) {
    hipLaunchKernelGGL((chamfer_nn_kernel<D, QPT>), dim3((unsigned)p.qtiles, (unsigned)p.splits, (unsigned)B), dim3(kThreads), 0, s, p1,
                       p2, N, M, p.chunk, p.splits, dist, idx, part_d2, part_idx, partials);
}

}  // namespace

extern "C" {

int64_t pn2_chamfer_nn_workspace_bytes(int B, int N, int M, int D) {
    if (B <= 0 || N <= 0 || M <= 0 || D <= 0 || D > kMaxD) return 0;
    return chamfer_work(make_plan(B, N, M), B, N, nullptr).bytes;
}

int pn2_chamfer_nn(const float *p1, const float *p2, int B, int N, int M, int D, float *dist, int64_t *idx, float *sum,
                   void *workspace, pn2_stream_t stream) {
    PN2_CHECK_ARG(p1 && p2 && dist && idx && workspace && B > 0 && B <= 65535 && N > 0 && M > 0 && D > 0);
    PN2_CHECK_ARG((int64_t)B * N < (int64_t)1 << 31 && (int64_t)N * D < (int64_t)1 << 31 && (int64_t)M * D < (int64_t)1 << 31);
    if (D > kMaxD) return PN2_EUNSUPPORTED;
    const Plan p = make_plan(B, N, M);
    const Work w = chamfer_work(p, B, N, workspace);
    double *want = sum ? w.partials : nullptr;
    hipStream_t s = pn2_s(stream);
#define PN2_CHAMFER_CASE(DD)                                                                                              \
    case DD:                                                                                                              \
        if (p.qpt == 4) launch_nn<DD, 4>(p, p1, p2, B, N, M, dist, idx, w.part_d2, w.part_idx, want, s);                      \
        else launch_nn<DD, 1>(p, p1, p2, B, N, M, dist, idx, w.part_d2, w.part_idx, want, s);                                 \
        break;
    switch (D) {
        PN2_CHAMFER_CASE(1) PN2_CHAMFER_CASE(2) PN2_CHAMFER_CASE(3) PN2_CHAMFER_CASE(4) PN2_CHAMFER_CASE(5) PN2_CHAMFER_CASE(6)
        PN2_CHAMFER_CASE(7) PN2_CHAMFER_CASE(8) PN2_CHAMFER_CASE(9) PN2_CHAMFER_CASE(10) PN2_CHAMFER_CASE(11) PN2_CHAMFER_CASE(12)
        PN2_CHAMFER_CASE(13) PN2_CHAMFER_CASE(14) PN2_CHAMFER_CASE(15) PN2_CHAMFER_CASE(16)
        default: return PN2_EUNSUPPORTED;
    }
#undef PN2_CHAMFER_CASE
    if (p.splits > 1)
        hipLaunchKernelGGL(chamfer_join_kernel, dim3((unsigned)p.partials), dim3(kThreads), 0, s, w.part_d2, w.part_idx, (int64_t)B * N,
                           p.splits, dist, idx, want);
    if (sum) hipLaunchKernelGGL(chamfer_sum_kernel, dim3(1), dim3(kThreads), 0, s, w.partials, p.partials, B, sum);
    return pn2_launch_status();
}

int pn2_chamfer_bwd(const float *p1, const float *p2, const float *dist, const int64_t *idx, const float *g, int B, int N, int M,
                    int D, float *dp1, float *dp2, pn2_stream_t stream) {
    PN2_CHECK_ARG(p1 && p2 && dist && idx && g && B > 0 && N > 0 && M > 0 && D > 0);
    if (D > kMaxD) return PN2_EUNSUPPORTED;
    if (dp1 == nullptr && dp2 == nullptr) return PN2_OK;
    const int64_t total = (int64_t)B * N * D;
    PN2_CHECK_ARG(pn2_cdiv(total, kThreads) < (int64_t)1 << 31);
    hipLaunchKernelGGL(chamfer_bwd_kernel, dim3((unsigned)pn2_cdiv(total, kThreads)), dim3(kThreads), 0, pn2_s(stream), p1, p2, dist,
                       idx, g, B, N, M, D, total, dp1, dp2);
    return pn2_launch_status();
}

}  // extern "C"
