// Plane RANSAC, least-squares refit and ground / plane classification: pn2_plane_ransac, pn2_plane_refit, pn2_plane_classify.  The
// rule is in include/pn2.h under "plane RANSAC" and in numpy in tests/plane_ref.py.
//
//   plane_hypothesis_kernel  one hypothesis per lane: three rows by the integer sampler, the plane through them in fp64, the flip,
//                            the angle test; four doubles per hypothesis to the workspace, four NaNs for an invalid one.
//   plane_score_kernel       one workgroup per (tile of kScoreTile rows, block of 256 hypotheses, cloud), ONE HYPOTHESIS PER LANE: its
//                            plane is four doubles in registers; the tile is staged once through LDS as three doubles a row (x = NaN
//                            for a row that takes no part or is not finite: its residual is NaN and fails the compare) and every
//                            lane reads the same address, a broadcast.  The lane's count is an integer in a register: there is no
//                            cross-lane reduction at all.  One int32 per (tile, hypothesis) goes to the workspace.
//   plane_select_kernel      one workgroup per cloud: the largest count, the lowest h among equals (ransac_select.h); the best
//                            hypothesis is the plane, zeros without one.
//   plane_accumulate_kernel  the tiled sum of tile_sum.h on ten words: one partial per tile; then one lane holds the totals, takes
//   plane_finish_kernel      pn2_sym_eig3 and writes the plane.
//   plane_count_kernel       the inliers of the final plane over the same tiles: a ballot and a popcount per wave, one int32 per tile.
//   plane_write_kernel       every workgroup adds those tile counts itself (integers: any order), decides min_inliers from the sum
//                            and writes dist and assign for its tile; tile 0 writes count and the status bit.
//   The order of every floating-point sum is a function of (B, N) alone (tile_sum.h).  No float atomics (the only atomics are the ORs into err),
//   no thread waits for another thread's write, nothing is allocated, plain launches.
//
// This file is built with -ffp-contract=off: every term is the separately rounded fp64 statement of the header.
#include <cmath>
#include "pn2_common.h"
#include "ransac_sample.h"
#include "ransac_select.h"
#include "sym_eig3.h"
#include "tile_sum.h"

namespace {

constexpr int kThreads = kSumThreads;                               // every kernel here; the count and write kernels walk tile_sum.h's tiles too
constexpr int kWaves = kThreads / PN2_WAVE;
constexpr int kSums = 10;                                           // count, sum q (3), sum q q^T (xx, xy, xz, yy, yz, zz)

struct Axis {
    double x, y, z;
};

__device__ __forceinline__ bool plane_takes_part(const int32_t *assign, int64_t at) { return assign == nullptr || assign[at] < 0; }

// n flipped so that n . axis >= 0; at exactly 0 the first non-zero component is made positive
__device__ __forceinline__ void plane_flip(double &nx, double &ny, double &nz, const Axis &a) {
    const double c = (nx * a.x + ny * a.y) + nz * a.z;
    const double lead = nx != 0.0 ? nx : (ny != 0.0 ? ny : nz);
    if (c < 0.0 || (c == 0.0 && lead < 0.0)) {
        nx = -nx;
        ny = -ny;
        nz = -nz;
    }
}

__device__ __forceinline__ double plane_residual(double nx, double ny, double nz, double d, double x, double y, double z) {
    return ((nx * x + ny * y) + nz * z) + d;
}

__global__ __launch_bounds__(kThreads) void plane_hypothesis_kernel(const float *__restrict__ pts, int ld, int N, const int64_t *__restrict__ n_points,
                                                                    const int32_t *__restrict__ assign, int H, unsigned long long seed, Axis axis,
                                                                    double cos_max, double *__restrict__ hyp) {
    const int b = blockIdx.y, h = blockIdx.x * kThreads + threadIdx.x;
    if (h >= H) return;
    const int n = pn2_rows_or_all(n_points, b, N);
    const double nan = __builtin_nan("");
    double nx = nan, ny = nan, nz = nan, d = nan;
    const int64_t r0 = ransac_sample(seed, b, h, 0, n), r1 = ransac_sample(seed, b, h, 1, n), r2 = ransac_sample(seed, b, h, 2, n);    // (ransac_sample.h)
    bool ok = n > 0 && r0 < n && r1 < n && r2 < n && r0 != r1 && r0 != r2 && r1 != r2;
    if (ok) {
        const int64_t base = (int64_t)b * N;
        ok = plane_takes_part(assign, base + r0) && plane_takes_part(assign, base + r1) && plane_takes_part(assign, base + r2);
    }
    if (ok) {
        const float *p0 = pts + ((int64_t)b * N + r0) * ld, *p1 = pts + ((int64_t)b * N + r1) * ld, *p2 = pts + ((int64_t)b * N + r2) * ld;
        const double x0 = (double)p0[0], y0 = (double)p0[1], z0 = (double)p0[2];
        const double ax = (double)p1[0] - x0, ay = (double)p1[1] - y0, az = (double)p1[2] - z0;
        const double bx = (double)p2[0] - x0, by = (double)p2[1] - y0, bz = (double)p2[2] - z0;
        ok = std::isfinite(x0) && std::isfinite(y0) && std::isfinite(z0) && std::isfinite(ax) && std::isfinite(ay) && std::isfinite(az) &&
             std::isfinite(bx) && std::isfinite(by) && std::isfinite(bz);                          // (p_0 and both differences finite: all three rows are)
        double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
        const double len2 = (cx * cx + cy * cy) + cz * cz;
        ok = ok && len2 > 0.0 && std::isfinite(len2);
        const double len = sqrt(len2);
        cx = cx / len;
        cy = cy / len;
        cz = cz / len;
        plane_flip(cx, cy, cz, axis);
        const double c = (cx * axis.x + cy * axis.y) + cz * axis.z;
        ok = ok && !(c < cos_max);
        if (ok) {
            nx = cx;
            ny = cy;
            nz = cz;
            d = -((cx * x0 + cy * y0) + cz * z0);
        }
    }
    double *o = hyp + ((int64_t)b * H + h) * 4;
    o[0] = nx;
    o[1] = ny;
    o[2] = nz;
    o[3] = d;
}

__global__ __launch_bounds__(kThreads) void plane_score_kernel(const float *__restrict__ pts, int ld, int N, const int64_t *__restrict__ n_points,
                                                               const int32_t *__restrict__ assign, int H, double threshold,
                                                               const double *__restrict__ hyp, int tiles, int32_t *__restrict__ tile_count,
                                                               int32_t *__restrict__ err) {
    __shared__ double s_x[kScoreTile], s_y[kScoreTile], s_z[kScoreTile];
    const int b = blockIdx.z, tile = blockIdx.x, t = threadIdx.x;
    const int n = pn2_rows_or_all(n_points, b, N);
    const int first = tile * kScoreTile;
    if (first >= n) return;                                         // (uniform over the workgroup; the select kernel does not read this tile)
    const int cnt = min(kScoreTile, n - first);
    bool bad = false;
    for (int k = t; k < cnt; k += kThreads) {
        const int64_t at = (int64_t)b * N + first + k;
        const float *p = pts + at * ld;
        const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
        const bool part = plane_takes_part(assign, at);
        const bool finite = std::isfinite(x) && std::isfinite(y) && std::isfinite(z);
        bad = bad || (part && !finite);
        s_x[k] = part && finite ? x : __builtin_nan("");
        s_y[k] = y;
        s_z[k] = z;
    }
    if (bad && err != nullptr && blockIdx.y == 0) atomicOr(err, PN2_PLANE_ERR_NONFINITE);
    __syncthreads();
    const int h = blockIdx.y * kThreads + t;
    if (h >= H) return;                                             // (after the only barrier)
    const double *q = hyp + ((int64_t)b * H + h) * 4;
    const double nx = q[0], ny = q[1], nz = q[2], d = q[3];
    int count = 0;
#pragma unroll 4
    for (int k = 0; k < cnt; ++k) {
        const double r = plane_residual(nx, ny, nz, d, s_x[k], s_y[k], s_z[k]);
        count += fabs(r) <= threshold ? 1 : 0;                      // (NaN fails)
    }
    tile_count[((int64_t)b * tiles + tile) * H + h] = count;
}

__global__ __launch_bounds__(kThreads) void plane_select_kernel(int N, const int64_t *__restrict__ n_points, int H, const double *__restrict__ hyp,
                                                                int tiles, const int32_t *__restrict__ tile_count, double *__restrict__ plane,
                                                                int32_t *__restrict__ hyp_count, int32_t *__restrict__ best_h,
                                                                int64_t *__restrict__ best_count, int32_t *__restrict__ status,
                                                                int32_t *__restrict__ err) {
    __shared__ unsigned long long s_key[kWaves];
    const int b = blockIdx.x;
    RansacBest best;
    if (!ransac_select(b, pn2_rows_or_all(n_points, b, N), H, hyp, 4, tiles, tile_count, hyp_count, s_key, best)) return;
    best_h[b] = best.h;
    best_count[b] = best.count;
    const bool none = !best.any || best.count < 3;
#pragma unroll
    for (int k = 0; k < 4; ++k) plane[(int64_t)b * 4 + k] = none ? 0.0 : hyp[((int64_t)b * H + best.h) * 4 + k];
    status[b] = none ? PN2_PLANE_NONE : 0;
    if (none && err != nullptr) atomicOr(err, PN2_PLANE_ERR_NONE);
}

// a row of the accumulate / count / write kernels: r against the plane, or NaN for a row that is not finite
__device__ __forceinline__ double plane_row_residual(const float *__restrict__ p, const double (&P)[4], double &x, double &y, double &z) {
    x = (double)p[0];
    y = (double)p[1];
    z = (double)p[2];
    const bool finite = std::isfinite(x) && std::isfinite(y) && std::isfinite(z);
    return finite ? plane_residual(P[0], P[1], P[2], P[3], x, y, z) : __builtin_nan("");
}

__global__ __launch_bounds__(kThreads) void plane_accumulate_kernel(const float *__restrict__ pts, int ld, int N, const int64_t *__restrict__ n_points,
                                                                    const int32_t *__restrict__ assign, double threshold,
                                                                    const double *__restrict__ plane, const int32_t *__restrict__ status,
                                                                    double *__restrict__ partial) {
    __shared__ double s_wave[kSumWaves][kSums];
    const int b = blockIdx.y, tile = blockIdx.x;
    if ((status[b] & PN2_PLANE_NONE) != 0) return;                  // (uniform over the workgroup)
    const int n = pn2_rows_or_all(n_points, b, N);
    double acc[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
    if ((int64_t)tile * kSumTile < n) {
        double P[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) P[k] = plane[(int64_t)b * 4 + k];
        const double sx = -P[3] * P[0], sy = -P[3] * P[1], sz = -P[3] * P[2];
#pragma nounroll
        for (int r = 0; r < kSumRows; ++r) {
            const int64_t i = pn2_tile_row(tile, r);
            if (i >= n) continue;
            const int64_t at = (int64_t)b * N + i;
            double x, y, z;
            const double res = plane_row_residual(pts + at * ld, P, x, y, z);
            if (!(fabs(res) <= threshold) || !plane_takes_part(assign, at)) continue;
            const double qx = x - sx, qy = y - sy, qz = z - sz;
            acc[0] = acc[0] + 1.0;
            acc[1] = acc[1] + qx;
            acc[2] = acc[2] + qy;
            acc[3] = acc[3] + qz;
            acc[4] = acc[4] + qx * qx;
            acc[5] = acc[5] + qx * qy;
            acc[6] = acc[6] + qx * qz;
            acc[7] = acc[7] + qy * qy;
            acc[8] = acc[8] + qy * qz;
            acc[9] = acc[9] + qz * qz;
        }
    }
    pn2_tile_partial(acc, s_wave, partial + ((int64_t)b * gridDim.x + tile) * kSums);
}

__global__ __launch_bounds__(kThreads) void plane_finish_kernel(int tiles, Axis axis, const double *__restrict__ partial, double *__restrict__ plane,
                                                                double *__restrict__ rmse, double *__restrict__ sums, int32_t *__restrict__ status) {
    __shared__ double s_chunk[kSumChunks][32];
    const int b = blockIdx.x;
    if ((status[b] & PN2_PLANE_NONE) != 0) return;
    double S[kSums];
    if (!pn2_tile_total(partial + (int64_t)b * tiles * kSums, tiles, s_chunk, S)) return;
#pragma unroll
    for (int q = 0; q < kSums; ++q) sums[(int64_t)b * kSums + q] = S[q];
    const double count = S[0];
    const double nx0 = plane[(int64_t)b * 4], ny0 = plane[(int64_t)b * 4 + 1], nz0 = plane[(int64_t)b * 4 + 2], d0 = plane[(int64_t)b * 4 + 3];
    const double sx = -d0 * nx0, sy = -d0 * ny0, sz = -d0 * nz0;
    const double mx = S[1] / count, my = S[2] / count, mz = S[3] / count;
    double l0, l1, l2, ux, uy, uz;
    pn2_sym_eig3(S[4] / count - mx * mx, S[5] / count - mx * my, S[6] / count - mx * mz, S[7] / count - my * my, S[8] / count - my * mz,
                 S[9] / count - mz * mz, l0, l1, l2, ux, uy, uz);
    if (count < 3.0 || !(l1 > 0.0) || !(std::isfinite(ux) && std::isfinite(uy) && std::isfinite(uz) && std::isfinite(l0))) {
        status[b] = status[b] | PN2_PLANE_DEGENERATE;               // the plane and rmse stay
        return;
    }
    plane_flip(ux, uy, uz, axis);
    plane[(int64_t)b * 4] = ux;
    plane[(int64_t)b * 4 + 1] = uy;
    plane[(int64_t)b * 4 + 2] = uz;
    plane[(int64_t)b * 4 + 3] = -((ux * (sx + mx) + uy * (sy + my)) + uz * (sz + mz));
    rmse[b] = sqrt(l0 > 0.0 ? l0 : 0.0);
}

__global__ __launch_bounds__(kThreads) void plane_count_kernel(const float *__restrict__ pts, int ld, int N, const int64_t *__restrict__ n_points,
                                                               const int32_t *__restrict__ assign, double threshold,
                                                               const double *__restrict__ plane, const int32_t *__restrict__ status,
                                                               int32_t *__restrict__ tile_count) {
    __shared__ int s_wave[kWaves];
    const int b = blockIdx.y, tile = blockIdx.x, t = threadIdx.x;
    if ((status[b] & PN2_PLANE_NONE) != 0) return;
    const int n = pn2_rows_or_all(n_points, b, N);
    int count = 0;
    if ((int64_t)tile * kSumTile < n) {
        double P[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) P[k] = plane[(int64_t)b * 4 + k];
#pragma nounroll
        for (int r = 0; r < kSumRows; ++r) {
            const int64_t i = pn2_tile_row(tile, r);
            bool in = false;
            if (i < n) {
                const int64_t at = (int64_t)b * N + i;
                double x, y, z;
                const double res = plane_row_residual(pts + at * ld, P, x, y, z);
                in = fabs(res) <= threshold && plane_takes_part(assign, at);
            }
            count += __popcll(__ballot(in));                        // (every lane of the wave holds the wave's count)
        }
    }
    if ((t & (PN2_WAVE - 1)) == 0) s_wave[t >> 6] = count;
    __syncthreads();
    if (t == 0) {
        int c = s_wave[0];
        for (int k = 1; k < kWaves; ++k) c += s_wave[k];
        tile_count[(int64_t)b * gridDim.x + tile] = c;
    }
}

__global__ __launch_bounds__(kThreads) void plane_write_kernel(const float *__restrict__ pts, int ld, int N, const int64_t *__restrict__ n_points,
                                                               int32_t *__restrict__ assign, int32_t plane_id, int64_t min_inliers, double threshold,
                                                               const double *__restrict__ plane, int32_t *__restrict__ status,
                                                               const int32_t *__restrict__ tile_count, float *__restrict__ dist,
                                                               int64_t *__restrict__ count) {
    __shared__ int64_t s_wave[kWaves];
    const int b = blockIdx.y, tile = blockIdx.x, t = threadIdx.x, tiles = gridDim.x;
    if ((status[b] & PN2_PLANE_NONE) != 0) return;
    int64_t c = 0;
    for (int k = t; k < tiles; k += kThreads) c += tile_count[(int64_t)b * tiles + k];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m, 64);
    if ((t & (PN2_WAVE - 1)) == 0) s_wave[t >> 6] = c;
    __syncthreads();
    c = 0;
    for (int k = 0; k < kWaves; ++k) c += s_wave[k];
    const bool mark = c >= min_inliers;
    if (tile == 0 && t == 0) {
        count[b] = c;
        if (!mark) status[b] = status[b] | PN2_PLANE_SMALL;         // (only this thread writes status[b]; the others read the NONE bit, which it keeps)
    }
    const int n = pn2_rows_or_all(n_points, b, N);
    double P[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) P[k] = plane[(int64_t)b * 4 + k];
#pragma nounroll
    for (int r = 0; r < kSumRows; ++r) {
        const int64_t i = pn2_tile_row(tile, r);
        if (i >= n) continue;
        const int64_t at = (int64_t)b * N + i;
        double x, y, z;
        const double res = plane_row_residual(pts + at * ld, P, x, y, z);
        if (dist != nullptr) dist[at] = (float)res;
        if (assign != nullptr && mark && fabs(res) <= threshold && assign[at] < 0) assign[at] = plane_id;
    }
}

bool plane_axis(const double *axis, Axis &a) {
    if (axis == nullptr || !(std::isfinite(axis[0]) && std::isfinite(axis[1]) && std::isfinite(axis[2]))) return false;
    const double len = sqrt((axis[0] * axis[0] + axis[1] * axis[1]) + axis[2] * axis[2]);
    if (!(len > 0.0) || !std::isfinite(len)) return false;
    a.x = axis[0] / len;
    a.y = axis[1] / len;
    a.z = axis[2] / len;
    return true;
}

struct PlaneWork {                  // (the refit's and the classification's parts come first: where they lie does not depend on H)
    double *partial;                // [B,row tiles,10]
    int32_t *rows;                  // [B,row tiles]
    double *hyp;                    // [B,H,4]
    int32_t *score;                 // [B,score tiles,H]
    int64_t bytes;
};

PlaneWork plane_work(int B, int64_t N, int H, void *base) {
    Pn2Arena a(base);
    const int64_t sum_tiles = B * pn2_cdiv(N, kSumTile), score_tiles = B * pn2_cdiv(N, kScoreTile);
    return {a.take<double>(sum_tiles * kSums), a.take<int32_t>(sum_tiles), a.take<double>((int64_t)B * H * 4), a.take<int32_t>(score_tiles * H), a.bytes()};
}

}  // namespace

extern "C" {

int64_t pn2_plane_workspace_bytes(int B, int N, int H) {
    if (!pn2_cloud_shape_ok(B, N) || H < 1 || H > 65536) return PN2_EINVAL;
    return plane_work(B, N, H, nullptr).bytes;
}

int pn2_plane_ransac(const float *pts, int ld, int B, int N, const int64_t *n_points, const int32_t *assign, int H, uint64_t seed,
                     const double *axis, double cos_max, double threshold, double *plane, int32_t *hyp_count, int32_t *best_h,
                     int64_t *best_count, int32_t *status, int32_t *err, void *workspace, pn2_stream_t stream) {
    PN2_CHECK_ARG(pts && plane && best_h && best_count && status && workspace);
    PN2_CHECK_ARG(pn2_cloud_shape_ok(B, N) && H >= 1 && H <= 65536 && ld >= 3 && ld <= 16);
    PN2_CHECK_ARG(std::isfinite(threshold) && threshold >= 0.0 && std::isfinite(cos_max));
    Axis a;
    PN2_CHECK_ARG(plane_axis(axis, a));
    PN2_CHECK_ARG(pn2_aligned(pts, 4) && pn2_aligned(assign, 4) && pn2_aligned(n_points, 8) && pn2_aligned(plane, 8) && pn2_aligned(hyp_count, 4));
    PN2_CHECK_ARG(pn2_aligned(best_h, 4) && pn2_aligned(best_count, 8) && pn2_aligned(status, 4) && pn2_aligned(err, 4) && pn2_aligned(workspace, 16));
    const PlaneWork w = plane_work(B, N, H, workspace);
    const int tiles = (int)pn2_cdiv(N, kScoreTile), hblocks = (int)pn2_cdiv(H, kThreads);
    PN2_CHECK_ARG(hblocks <= 65535);
    const hipStream_t s = pn2_s(stream);
    hipLaunchKernelGGL(plane_hypothesis_kernel, dim3((unsigned)hblocks, (unsigned)B), dim3(kThreads), 0, s, pts, ld, N, n_points, assign, H,
                       (unsigned long long)seed, a, cos_max, w.hyp);
    hipLaunchKernelGGL(plane_score_kernel, dim3((unsigned)tiles, (unsigned)hblocks, (unsigned)B), dim3(kThreads), 0, s, pts, ld, N, n_points, assign,
                       H, threshold, w.hyp, tiles, w.score, err);
    hipLaunchKernelGGL(plane_select_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, N, n_points, H, w.hyp, tiles, w.score, plane, hyp_count,
                       best_h, best_count, status, err);
    return pn2_launch_status();
}

int pn2_plane_refit(const float *pts, int ld, int B, int N, const int64_t *n_points, const int32_t *assign, const double *axis,
                    double threshold, double *plane, double *rmse, double *sums, int32_t *status, void *workspace, pn2_stream_t stream) {
    PN2_CHECK_ARG(pts && plane && rmse && sums && status && workspace);
    PN2_CHECK_ARG(pn2_cloud_shape_ok(B, N) && ld >= 3 && ld <= 16);
    PN2_CHECK_ARG(std::isfinite(threshold) && threshold >= 0.0);
    Axis a;
    PN2_CHECK_ARG(plane_axis(axis, a));
    PN2_CHECK_ARG(pn2_aligned(pts, 4) && pn2_aligned(assign, 4) && pn2_aligned(n_points, 8) && pn2_aligned(plane, 8) && pn2_aligned(rmse, 8));
    PN2_CHECK_ARG(pn2_aligned(sums, 8) && pn2_aligned(status, 4) && pn2_aligned(workspace, 16));
    const PlaneWork w = plane_work(B, N, 1, workspace);
    const int tiles = (int)pn2_cdiv(N, kSumTile);
    const hipStream_t s = pn2_s(stream);
    hipLaunchKernelGGL(plane_accumulate_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(kThreads), 0, s, pts, ld, N, n_points, assign, threshold,
                       plane, status, w.partial);
    hipLaunchKernelGGL(plane_finish_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, tiles, a, w.partial, plane, rmse, sums, status);
    return pn2_launch_status();
}

int pn2_plane_classify(const float *pts, int ld, int B, int N, const int64_t *n_points, int32_t *assign, int32_t plane_id, int64_t min_inliers,
                       double threshold, const double *plane, int32_t *status, float *dist, int64_t *count, void *workspace,
                       pn2_stream_t stream) {
    PN2_CHECK_ARG(pts && plane && status && count && workspace);
    PN2_CHECK_ARG(pn2_cloud_shape_ok(B, N) && ld >= 3 && ld <= 16);
    PN2_CHECK_ARG(std::isfinite(threshold) && threshold >= 0.0 && plane_id >= 0);
    PN2_CHECK_ARG(pn2_aligned(pts, 4) && pn2_aligned(assign, 4) && pn2_aligned(n_points, 8) && pn2_aligned(plane, 8) && pn2_aligned(status, 4));
    PN2_CHECK_ARG(pn2_aligned(dist, 4) && pn2_aligned(count, 8) && pn2_aligned(workspace, 16));
    const PlaneWork w = plane_work(B, N, 1, workspace);
    const int tiles = (int)pn2_cdiv(N, kSumTile);
    const hipStream_t s = pn2_s(stream);
    const dim3 by_tile((unsigned)tiles, (unsigned)B);
    hipLaunchKernelGGL(plane_count_kernel, by_tile, dim3(kThreads), 0, s, pts, ld, N, n_points, assign, threshold, plane, status, w.rows);
    hipLaunchKernelGGL(plane_write_kernel, by_tile, dim3(kThreads), 0, s, pts, ld, N, n_points, assign, plane_id, min_inliers, threshold, plane,
                       status, w.rows, dist, count);
    return pn2_launch_status();
}

}  // extern "C"
