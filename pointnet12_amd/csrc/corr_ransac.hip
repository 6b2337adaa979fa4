// Correspondence RANSAC and its least-squares refit: the rigid transform that takes the source rows of a pair list onto their target
// rows: pn2_corr_ransac, pn2_corr_refit.  The rule is in include/pn2.h under "correspondence RANSAC" and in numpy in
// tests/corr_ransac_ref.py.
//
//   corr_hypothesis_kernel  one hypothesis per lane: three pair rows by the integer sampler (ransac_sample.h), the index, edge and
//                           triangle tests, the transform by the triad rule in fp64; twelve doubles per hypothesis ([R | t], row
//                           major), twelve NaNs for an invalid one.
//   corr_score_kernel       plane_score_kernel's shape: one workgroup per (tile of kScoreTile pairs, block of 256 hypotheses, cloud),
//                           ONE HYPOTHESIS PER LANE with its twelve doubles in registers; the tile is staged once through LDS as six
//                           doubles a pair (p_x = NaN for a pair that is out of range or not finite: its d2 is NaN and fails the
//                           compare) and broadcast-read; an integer count per lane, no cross-lane reduction.
//   corr_select_kernel      the largest count, the lowest h among equals (ransac_select.h); the best hypothesis is T, the identity
//                           without one.
//   corr_accumulate_kernel  the tiled sum of tile_sum.h on seventeen words, a pair where it says row: one partial per tile; then one
//   corr_finish_kernel      lane holds the totals and solves by Horn's quaternion method (sym_eig4.h: cyclic Jacobi on the
//                           symmetric 4 x 4, a fixed number of sweeps).
//   The order of every floating-point sum is a function of (B, N) alone (tile_sum.h).  No float atomics (the only atomics are the ORs into err),
//   no thread waits for another thread's write, nothing is allocated, plain launches.
//
// This file is built with -ffp-contract=off: every term is the separately rounded fp64 statement of the header.
#include <cmath>
#include "pn2_common.h"
#include "ransac_sample.h"
#include "ransac_select.h"
#include "rigid.h"
#include "sym_eig4.h"
#include "tile_sum.h"

namespace {

constexpr int kThreads = kSumThreads;                               // every kernel here
constexpr int kWaves = kThreads / PN2_WAVE;
constexpr int kSums = PN2_CORR_SUMS;                                // count, sum p (3), sum q (3), sum p q^T (9, p major), sum d2

__device__ __forceinline__ double corr_len(const double (&a)[3], const double (&b)[3]) {
    const double x = b[0] - a[0], y = b[1] - a[1], z = b[2] - a[2];
    return sqrt((x * x + y * y) + z * z);
}

__device__ __forceinline__ bool corr_edge_ok(double lp, double lq, double edge_ratio) {
    const double lo = lp < lq ? lp : lq, hi = lp < lq ? lq : lp;
    return lp > 0.0 && lq > 0.0 && lo >= edge_ratio * hi;           // (a NaN fails)
}

// the triad frame of one side: F[c] = e_(c+1) as a vector (the columns of the header's F), c = the centre
__device__ __forceinline__ bool corr_frame(const double (&a0)[3], const double (&a1)[3], const double (&a2)[3], double l01, double (&F)[3][3],
                                           double (&c)[3]) {
    double v[3], w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        F[0][k] = (a1[k] - a0[k]) / l01;
        v[k] = a2[k] - a0[k];
        c[k] = ((a0[k] + a1[k]) + a2[k]) / 3.0;
    }
    w[0] = F[0][1] * v[2] - F[0][2] * v[1];
    w[1] = F[0][2] * v[0] - F[0][0] * v[2];
    w[2] = F[0][0] * v[1] - F[0][1] * v[0];
    const double len = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) F[2][k] = w[k] / len;
    F[1][0] = F[2][1] * F[0][2] - F[2][2] * F[0][1];
    F[1][1] = F[2][2] * F[0][0] - F[2][0] * F[0][2];
    F[1][2] = F[2][0] * F[0][1] - F[2][1] * F[0][0];
    return len > 0.0 && std::isfinite(len);
}

__device__ __forceinline__ bool corr_load(const float *__restrict__ p, double (&a)[3]) {
    a[0] = (double)p[0];
    a[1] = (double)p[1];
    a[2] = (double)p[2];
    return std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2]);
}

// d2 of a pair under T = [R | t]: e = (R p + t) - q
__device__ __forceinline__ double corr_d2(const double (&T)[12], double px, double py, double pz, double qx, double qy, double qz) {
    const double ex = pn2_rigid_apply<0>(T, px, py, pz) - qx;
    const double ey = pn2_rigid_apply<1>(T, px, py, pz) - qy;
    const double ez = pn2_rigid_apply<2>(T, px, py, pz) - qz;
    return (ex * ex + ey * ey) + ez * ez;
}

__global__ __launch_bounds__(kThreads) void corr_hypothesis_kernel(const float *__restrict__ src, int lds, const float *__restrict__ tgt, int ldt, int N,
                                                                   int M, const int64_t *__restrict__ pair_src, const int64_t *__restrict__ pair_tgt,
                                                                   const int64_t *__restrict__ count, int H, unsigned long long seed,
                                                                   double edge_ratio, double *__restrict__ hyp) {
    const int b = blockIdx.y, h = blockIdx.x * kThreads + threadIdx.x;
    if (h >= H) return;
    const int n = pn2_rows_or_all(count, b, N);
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = __builtin_nan("");
    const int64_t r0 = ransac_sample(seed, b, h, 0, n), r1 = ransac_sample(seed, b, h, 1, n), r2 = ransac_sample(seed, b, h, 2, n);
    bool ok = n >= 3 && r0 < n && r1 < n && r2 < n && r0 != r1 && r0 != r2 && r1 != r2;
    int64_t s0 = 0, s1 = 0, s2 = 0, t0 = 0, t1 = 0, t2 = 0;
    if (ok) {
        const int64_t base = (int64_t)b * N;
        s0 = pair_src[base + r0], s1 = pair_src[base + r1], s2 = pair_src[base + r2];
        t0 = pair_tgt[base + r0], t1 = pair_tgt[base + r1], t2 = pair_tgt[base + r2];
        ok = s0 >= 0 && s0 < N && s1 >= 0 && s1 < N && s2 >= 0 && s2 < N && t0 >= 0 && t0 < M && t1 >= 0 && t1 < M && t2 >= 0 && t2 < M;
        ok = ok && s0 != s1 && s0 != s2 && s1 != s2 && t0 != t1 && t0 != t2 && t1 != t2;
    }
    if (ok) {
        double p0[3], p1[3], p2[3], q0[3], q1[3], q2[3];
        ok = corr_load(src + ((int64_t)b * N + s0) * lds, p0);
        ok = corr_load(src + ((int64_t)b * N + s1) * lds, p1) && ok;
        ok = corr_load(src + ((int64_t)b * N + s2) * lds, p2) && ok;
        ok = corr_load(tgt + ((int64_t)b * M + t0) * ldt, q0) && ok;
        ok = corr_load(tgt + ((int64_t)b * M + t1) * ldt, q1) && ok;
        ok = corr_load(tgt + ((int64_t)b * M + t2) * ldt, q2) && ok;
        const double lp01 = corr_len(p0, p1), lq01 = corr_len(q0, q1);
        ok = ok && corr_edge_ok(lp01, lq01, edge_ratio) && corr_edge_ok(corr_len(p0, p2), corr_len(q0, q2), edge_ratio) &&
             corr_edge_ok(corr_len(p1, p2), corr_len(q1, q2), edge_ratio);
        double Fp[3][3], Fq[3][3], cp[3], cq[3], R[12];
        ok = corr_frame(p0, p1, p2, lp01, Fp, cp) && ok;
        ok = corr_frame(q0, q1, q2, lq01, Fq, cq) && ok;
        bool finite = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int c = 0; c < 3; ++c) R[a * 4 + c] = (Fq[0][a] * Fp[0][c] + Fq[1][a] * Fp[1][c]) + Fq[2][a] * Fp[2][c];
            R[a * 4 + 3] = cq[a] - ((R[a * 4] * cp[0] + R[a * 4 + 1] * cp[1]) + R[a * 4 + 2] * cp[2]);
#pragma unroll
            for (int c = 0; c < 4; ++c) finite = finite && std::isfinite(R[a * 4 + c]);
        }
        if (ok && finite) {
#pragma unroll
            for (int k = 0; k < 12; ++k) T[k] = R[k];
        }
    }
    double *o = hyp + ((int64_t)b * H + h) * 12;
#pragma unroll
    for (int k = 0; k < 12; ++k) o[k] = T[k];
}

// one pair of a cloud: its six doubles, p_x = NaN for a pair that takes no part; the err bits it earns
__device__ __forceinline__ int corr_pair(const float *__restrict__ src, int lds, const float *__restrict__ tgt, int ldt, int N, int M, int b,
                                         int64_t s, int64_t t, double (&p)[3], double (&q)[3]) {
    int bits = 0;
    p[0] = __builtin_nan("");
    p[1] = p[2] = q[0] = q[1] = q[2] = 0.0;
    if (s < 0 || s >= N || t < 0 || t >= M) return PN2_CORR_ERR_PAIR;
    const bool fp = corr_load(src + ((int64_t)b * N + s) * lds, p), fq = corr_load(tgt + ((int64_t)b * M + t) * ldt, q);
    if (!(fp && fq)) {
        bits = PN2_CORR_ERR_NONFINITE;
        p[0] = __builtin_nan("");
    }
    return bits;
}

__global__ __launch_bounds__(kThreads) void corr_score_kernel(const float *__restrict__ src, int lds, const float *__restrict__ tgt, int ldt, int N, int M,
                                                              const int64_t *__restrict__ pair_src, const int64_t *__restrict__ pair_tgt,
                                                              const int64_t *__restrict__ count, int H, double thr2, const double *__restrict__ hyp,
                                                              int tiles, int32_t *__restrict__ tile_count, int32_t *__restrict__ err) {
    __shared__ double s_p[3][kScoreTile], s_q[3][kScoreTile];
    const int b = blockIdx.z, tile = blockIdx.x, t = threadIdx.x;
    const int n = pn2_rows_or_all(count, b, N);
    const int first = tile * kScoreTile;
    if (first >= n) return;                                         // (uniform over the workgroup; the select kernel does not read this tile)
    const int cnt = min(kScoreTile, n - first);
    int bits = 0;
    for (int k = t; k < cnt; k += kThreads) {
        const int64_t at = (int64_t)b * N + first + k;
        double p[3], q[3];
        bits |= corr_pair(src, lds, tgt, ldt, N, M, b, pair_src[at], pair_tgt[at], p, q);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            s_p[a][k] = p[a];
            s_q[a][k] = q[a];
        }
    }
    if (bits != 0 && err != nullptr && blockIdx.y == 0) atomicOr(err, bits);
    __syncthreads();
    const int h = blockIdx.y * kThreads + t;
    if (h >= H) return;                                             // (after the only barrier)
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = hyp[((int64_t)b * H + h) * 12 + k];
    int c = 0;
#pragma unroll 2
    for (int k = 0; k < cnt; ++k) c += corr_d2(T, s_p[0][k], s_p[1][k], s_p[2][k], s_q[0][k], s_q[1][k], s_q[2][k]) <= thr2 ? 1 : 0;      // (NaN fails)
    tile_count[((int64_t)b * tiles + tile) * H + h] = c;
}

__global__ __launch_bounds__(kThreads) void corr_select_kernel(int N, const int64_t *__restrict__ count, int H, const double *__restrict__ hyp, int tiles,
                                                               const int32_t *__restrict__ tile_count, double *__restrict__ T,
                                                               int32_t *__restrict__ hyp_count, int32_t *__restrict__ best_h,
                                                               int64_t *__restrict__ best_count, int32_t *__restrict__ status,
                                                               int32_t *__restrict__ err) {
    __shared__ unsigned long long s_key[kWaves];
    const int b = blockIdx.x;
    RansacBest best;
    if (!ransac_select(b, pn2_rows_or_all(count, b, N), H, hyp, 12, tiles, tile_count, hyp_count, s_key, best)) return;
    best_h[b] = best.h;
    best_count[b] = best.count;
    const bool none = !best.any || best.count < 3;
#pragma unroll
    for (int k = 0; k < 12; ++k) T[(int64_t)b * 12 + k] = none ? ((k & 3) == (k >> 2) ? 1.0 : 0.0) : hyp[((int64_t)b * H + best.h) * 12 + k];
    status[b] = none ? PN2_CORR_NONE : 0;
    if (none && err != nullptr) atomicOr(err, PN2_CORR_ERR_NONE);
}

__global__ __launch_bounds__(kThreads) void corr_accumulate_kernel(const float *__restrict__ src, int lds, const float *__restrict__ tgt, int ldt, int N,
                                                                   int M, const int64_t *__restrict__ pair_src, const int64_t *__restrict__ pair_tgt,
                                                                   const int64_t *__restrict__ count, double thr2, const double *__restrict__ Tin,
                                                                   const int32_t *__restrict__ status, double *__restrict__ partial) {
    __shared__ double s_wave[kSumWaves][kSums];
    const int b = blockIdx.y, tile = blockIdx.x;
    if ((status[b] & PN2_CORR_NONE) != 0) return;                   // (uniform over the workgroup)
    const int n = pn2_rows_or_all(count, b, N);
    double acc[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
    if ((int64_t)tile * kSumTile < n) {
        double T[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = Tin[(int64_t)b * 12 + k];
#pragma nounroll
        for (int r = 0; r < kSumRows; ++r) {
            const int64_t i = pn2_tile_row(tile, r);
            if (i >= n) continue;
            const int64_t at = (int64_t)b * N + i;
            double p[3], q[3];
            corr_pair(src, lds, tgt, ldt, N, M, b, pair_src[at], pair_tgt[at], p, q);
            const double d2 = corr_d2(T, p[0], p[1], p[2], q[0], q[1], q[2]);
            if (!(d2 <= thr2)) continue;
            acc[0] = acc[0] + 1.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                acc[1 + a] = acc[1 + a] + p[a];
                acc[4 + a] = acc[4 + a] + q[a];
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[7 + 3 * a + c] = acc[7 + 3 * a + c] + p[a] * q[c];
            }
            acc[16] = acc[16] + d2;
        }
    }
    pn2_tile_partial(acc, s_wave, partial + ((int64_t)b * gridDim.x + tile) * kSums);
}

__global__ __launch_bounds__(kThreads) void corr_finish_kernel(int tiles, int flags, const double *__restrict__ partial, double *__restrict__ T,
                                                               int64_t *__restrict__ inliers, double *__restrict__ rmse, double *__restrict__ sums,
                                                               int32_t *__restrict__ status) {
    __shared__ double s_chunk[kSumChunks][32];
    const int b = blockIdx.x;
    if ((status[b] & PN2_CORR_NONE) != 0) return;
    double S[kSums];
    if (!pn2_tile_total(partial + (int64_t)b * tiles * kSums, tiles, s_chunk, S)) return;
#pragma unroll
    for (int q = 0; q < kSums; ++q) sums[(int64_t)b * kSums + q] = S[q];
    const double n = S[0];
    inliers[b] = (int64_t)n;
    rmse[b] = n > 0.0 ? sqrt(S[16] / n) : 0.0;
    if ((flags & PN2_CORR_EVAL_ONLY) != 0) return;
    // Horn: S_ab = sum p_a q_b - (sum p_a)(sum q_b) / n, the symmetric 4 x 4 N(S), its largest eigenvector as a quaternion
    double C[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int e = 0; e < 3; ++e) C[a][e] = S[7 + 3 * a + e] - (S[1 + a] * S[4 + e]) / n;
    double A[4][4], u[4];
    A[0][0] = (C[0][0] + C[1][1]) + C[2][2];
    A[1][1] = (C[0][0] - C[1][1]) - C[2][2];
    A[2][2] = (C[1][1] - C[0][0]) - C[2][2];
    A[3][3] = (C[2][2] - C[0][0]) - C[1][1];
    A[0][1] = A[1][0] = C[1][2] - C[2][1];
    A[0][2] = A[2][0] = C[2][0] - C[0][2];
    A[0][3] = A[3][0] = C[0][1] - C[1][0];
    A[1][2] = A[2][1] = C[0][1] + C[1][0];
    A[1][3] = A[3][1] = C[2][0] + C[0][2];
    A[2][3] = A[3][2] = C[1][2] + C[2][1];
    pn2_sym_eig4_largest(A, u);
    const double len = sqrt(((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) + u[3] * u[3]);
    const bool neg = u[0] / len < 0.0;
    const double w = neg ? -(u[0] / len) : u[0] / len, x = neg ? -(u[1] / len) : u[1] / len, y = neg ? -(u[2] / len) : u[2] / len,
                 z = neg ? -(u[3] / len) : u[3] / len;
    double R[12];
    R[0] = ((w * w + x * x) - y * y) - z * z;
    R[1] = 2.0 * (x * y - w * z);
    R[2] = 2.0 * (x * z + w * y);
    R[4] = 2.0 * (x * y + w * z);
    R[5] = ((w * w - x * x) + y * y) - z * z;
    R[6] = 2.0 * (y * z - w * x);
    R[8] = 2.0 * (x * z - w * y);
    R[9] = 2.0 * (y * z + w * x);
    R[10] = ((w * w - x * x) - y * y) + z * z;
    const double pm[3] = {S[1] / n, S[2] / n, S[3] / n};
    bool finite = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        R[a * 4 + 3] = S[4 + a] / n - ((R[a * 4] * pm[0] + R[a * 4 + 1] * pm[1]) + R[a * 4 + 2] * pm[2]);
#pragma unroll
        for (int e = 0; e < 4; ++e) finite = finite && std::isfinite(R[a * 4 + e]);
    }
    if (n < 3.0 || !finite) {
        status[b] = status[b] | PN2_CORR_DEGENERATE;                // T stays
        return;
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) T[(int64_t)b * 12 + e] = R[e];
}

struct CorrWork {                   // (the refit's part comes first: where it lies does not depend on H)
    double *partial, *hyp;          // [B,row tiles,17]; [B,H,12]
    int32_t *score;                 // [B,score tiles,H]
    int64_t bytes;
};

CorrWork corr_work(int B, int64_t N, int H, void *base) {
    Pn2Arena a(base);
    return {a.take<double>(B * pn2_cdiv(N, kSumTile) * kSums), a.take<double>((int64_t)B * H * 12), a.take<int32_t>(B * pn2_cdiv(N, kScoreTile) * H), a.bytes()};
}

bool corr_clouds_ok(const float *src, int lds, const float *tgt, int ldt, int B, int N, int M, const int64_t *pair_src, const int64_t *pair_tgt,
                    const int64_t *count, double threshold) {
    return src && tgt && pair_src && pair_tgt && pn2_cloud_shape_ok(B, N) && pn2_cloud_shape_ok(B, M) && lds >= 3 && lds <= 16 && ldt >= 3 && ldt <= 16 &&
           std::isfinite(threshold) && threshold >= 0.0 && pn2_aligned(src, 4) && pn2_aligned(tgt, 4) && pn2_aligned(pair_src, 8) &&
           pn2_aligned(pair_tgt, 8) && pn2_aligned(count, 8);
}

}  // namespace

extern "C" {

int64_t pn2_corr_workspace_bytes(int B, int N, int H) {
    if (!pn2_cloud_shape_ok(B, N) || H < 1 || H > 65536) return PN2_EINVAL;
    return corr_work(B, N, H, nullptr).bytes;
}

int pn2_corr_ransac(const float *src, int lds, const float *tgt, int ldt, int B, int N, int M, const int64_t *pair_src, const int64_t *pair_tgt,
                    const int64_t *count, int H, uint64_t seed, double edge_ratio, double threshold, double *T, double *hyp_T, int32_t *hyp_count,
                    int32_t *best_h, int64_t *best_count, int32_t *status, int32_t *err, void *workspace, pn2_stream_t stream) {
    PN2_CHECK_ARG(corr_clouds_ok(src, lds, tgt, ldt, B, N, M, pair_src, pair_tgt, count, threshold));
    PN2_CHECK_ARG(T && best_h && best_count && status && workspace && H >= 1 && H <= 65536 && edge_ratio >= 0.0 && edge_ratio <= 1.0);
    PN2_CHECK_ARG(pn2_aligned(T, 8) && pn2_aligned(hyp_T, 8) && pn2_aligned(hyp_count, 4) && pn2_aligned(best_h, 4) && pn2_aligned(best_count, 8) &&
                  pn2_aligned(status, 4) && pn2_aligned(err, 4) && pn2_aligned(workspace, 16));
    const CorrWork w = corr_work(B, N, H, workspace);
    double *hyp = hyp_T != nullptr ? hyp_T : w.hyp;
    const int tiles = (int)pn2_cdiv(N, kScoreTile), hblocks = (int)pn2_cdiv(H, kThreads);
    const hipStream_t s = pn2_s(stream);
    hipLaunchKernelGGL(corr_hypothesis_kernel, dim3((unsigned)hblocks, (unsigned)B), dim3(kThreads), 0, s, src, lds, tgt, ldt, N, M, pair_src, pair_tgt,
                       count, H, (unsigned long long)seed, edge_ratio, hyp);
    hipLaunchKernelGGL(corr_score_kernel, dim3((unsigned)tiles, (unsigned)hblocks, (unsigned)B), dim3(kThreads), 0, s, src, lds, tgt, ldt, N, M,
                       pair_src, pair_tgt, count, H, threshold * threshold, hyp, tiles, w.score, err);
    hipLaunchKernelGGL(corr_select_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, N, count, H, hyp, tiles, w.score, T, hyp_count, best_h, best_count,
                       status, err);
    return pn2_launch_status();
}

int pn2_corr_refit(const float *src, int lds, const float *tgt, int ldt, int B, int N, int M, const int64_t *pair_src, const int64_t *pair_tgt,
                   const int64_t *count, double threshold, int flags, double *T, int64_t *inliers, double *rmse, double *sums, int32_t *status,
                   void *workspace, pn2_stream_t stream) {
    PN2_CHECK_ARG(corr_clouds_ok(src, lds, tgt, ldt, B, N, M, pair_src, pair_tgt, count, threshold));
    PN2_CHECK_ARG(T && inliers && rmse && sums && status && workspace && (flags & ~PN2_CORR_EVAL_ONLY) == 0);
    PN2_CHECK_ARG(pn2_aligned(T, 8) && pn2_aligned(inliers, 8) && pn2_aligned(rmse, 8) && pn2_aligned(sums, 8) && pn2_aligned(status, 4) &&
                  pn2_aligned(workspace, 16));
    const CorrWork w = corr_work(B, N, 1, workspace);
    const int tiles = (int)pn2_cdiv(N, kSumTile);
    const hipStream_t s = pn2_s(stream);
    hipLaunchKernelGGL(corr_accumulate_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(kThreads), 0, s, src, lds, tgt, ldt, N, M, pair_src, pair_tgt,
                       count, threshold * threshold, T, status, w.partial);
    hipLaunchKernelGGL(corr_finish_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, tiles, flags, w.partial, T, inliers, rmse, sums, status);
    return pn2_launch_status();
}

}  // extern "C"
