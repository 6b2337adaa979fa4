// Rigid scan registration: pn2_icp_step does ONE Gauss-Newton iteration of point-to-plane or point-to-point ICP for B clouds against
// targets that pn2_grid_build has binned.  The rule is in include/pn2.h under "ICP step" and in numpy in tests/icp_ref.py.
//
//   icp_accumulate_kernel  one workgroup per tile of source rows, one row per lane (the tiled sum of tile_sum.h on kIcpWords words):
//                          the row through T in fp64 (rigid.h), rounded to fp32, the K = 1 walk over the 27 cells (grid_walk.h: the
//                          walk and the arithmetic of pn2_grid_knn), the residual and its Jacobian in fp64, the 28 products added
//                          to 28 accumulators in registers, the row counted in a 29th; ONE partial per tile.  Neither the
//                          transformed cloud nor a distance per row goes to memory.  A tile at or beyond the cloud's count writes
//                          zeros (the workspace arrives holding anything); the tiles of a frozen cloud return at once.
//   icp_finish_kernel      one workgroup per cloud: the total of the partials; ONE lane then does the 6 x 6 Cholesky solve, the
//                          rotation update and the status on scalars.
//   The order of every sum is a function of (B, N) alone: tile_sum.h states it.  No float atomics (the only atomics are the ORs
//   into err), no thread waits for another thread's write, nothing is allocated, two plain launches.
//
// This file is built with -ffp-contract=off: every term is the separately rounded fp64 statement of the header.
#include <cmath>
#include "grid_walk.h"
#include "rigid.h"
#include "tile_sum.h"

namespace {

static_assert(kThreads == kSumThreads, "the walk's workgroup is the tiled sum's");
constexpr int kIcpSums = 28;                                        // A's upper triangle (21), b (6), E
constexpr int kIcpWords = kIcpSums + 1;                             // ... and the count, as a double (an integer below 2^31: exact)

// the 28 products of one residual: J_k J_l for k <= l row-major, J_k r, r r -- each one multiplication and one addition
__device__ __forceinline__ void icp_add_terms(double (&acc)[kIcpWords], const double (&J)[6], double r) {
    int at = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int l = k; l < 6; ++l) {
            acc[at] = acc[at] + J[k] * J[l];
            ++at;
        }
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[21 + k] = acc[21 + k] + J[k] * r;
    acc[27] = acc[27] + r * r;
}

// one residual along n at the transformed point p with e = p - q
__device__ __forceinline__ void icp_residual(double (&acc)[kIcpWords], double px, double py, double pz, double ex, double ey, double ez,
                                             double nx, double ny, double nz) {
    const double r = (nx * ex + ny * ey) + nz * ez;
    const double J[6] = {py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz};
    icp_add_terms(acc, J, r);
}

template <int METRIC>
__global__ __launch_bounds__(kThreads) void icp_accumulate_kernel(const float *__restrict__ src, int lds, int N, const int64_t *__restrict__ n_src,
                                                                  const float *__restrict__ tgt, int ldt, int M,
                                                                  const float *__restrict__ nrm, int ldn, Grid grid, Work w, float max_d2,
                                                                  int eval, const double *__restrict__ T, const int32_t *__restrict__ status,
                                                                  int64_t *__restrict__ corr, int32_t *__restrict__ err,
                                                                  double *__restrict__ partial) {
    __shared__ double s_wave[kSumWaves][kIcpWords];
    const int b = blockIdx.y, tile = blockIdx.x;
    if (!eval && (status[b] & (PN2_ICP_CONVERGED | PN2_ICP_SINGULAR)) != 0) return;        // frozen: not walked (uniform over the workgroup)
    const int n = pn2_rows_or_all(n_src, b, N);
    double acc[kIcpWords];
#pragma unroll
    for (int k = 0; k < kIcpSums; ++k) acc[k] = 0.0;
    int rows = 0;
    if ((int64_t)tile * kSumTile < n) {
        double R[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) R[k] = T[(int64_t)b * 12 + k];
#pragma nounroll
        for (int r = 0; r < kSumRows; ++r) {
            const int64_t i = pn2_tile_row(tile, r);
            if (i >= n) continue;
            const float *s = src + ((int64_t)b * N + i) * lds;
            const double sx = (double)s[0], sy = (double)s[1], sz = (double)s[2];
            const double px = pn2_rigid_apply<0>(R, sx, sy, sz), py = pn2_rigid_apply<1>(R, sx, sy, sz), pz = pn2_rigid_apply<2>(R, sx, sy, sz);
            float bd[1] = {INFINITY};
            int bi[1] = {M};
            int took = 0;
            if (!pn2_grid_walk<1>((float)px, (float)py, (float)pz, grid, w, b, M, max_d2, bd, bi, took) && err != nullptr)
                atomicOr(err, PN2_ICP_ERR_QUERY);
            int j = bi[0];
            if (j < 0 || j > M) j = M;                              // (never after a build: the index is used as an address below)
            if (corr != nullptr) corr[(int64_t)b * N + i] = j;
            if (j >= M) continue;
            const float *q = tgt + ((int64_t)b * M + j) * ldt;
            const double ex = px - (double)q[0], ey = py - (double)q[1], ez = pz - (double)q[2];
            if (METRIC == PN2_ICP_PLANE) {
                const float *nf = nrm + ((int64_t)b * M + j) * ldn;
                const double nx = (double)nf[0], ny = (double)nf[1], nz = (double)nf[2];
                if (!(std::isfinite(nx) && std::isfinite(ny) && std::isfinite(nz)) || (nx == 0.0 && ny == 0.0 && nz == 0.0)) continue;
                icp_residual(acc, px, py, pz, ex, ey, ez, nx, ny, nz);
            } else {
                icp_residual(acc, px, py, pz, ex, ey, ez, 1.0, 0.0, 0.0);
                icp_residual(acc, px, py, pz, ex, ey, ez, 0.0, 1.0, 0.0);
                icp_residual(acc, px, py, pz, ex, ey, ez, 0.0, 0.0, 1.0);
            }
            ++rows;
        }
    }
    acc[kIcpSums] = (double)rows;
    pn2_tile_partial(acc, s_wave, partial + ((int64_t)b * gridDim.x + tile) * kIcpWords);
}

constexpr int icp_upper(int k, int l) { return k * 6 - k * (k - 1) / 2 + (l - k); }        // A_kl, k <= l, in the 21 words
constexpr int icp_lower(int i, int j) { return i * (i + 1) / 2 + j; }                      // L_ij, j <= i
static_assert(icp_upper(5, 5) == 20 && icp_upper(1, 1) == 6 && icp_lower(5, 5) == 20, "two triangles of 21 words");

// A x = -b by Cholesky in index order; false: a pivot at or below 2^-40 of its diagonal entry, or not finite
__device__ __forceinline__ bool icp_solve(const double (&S)[kIcpWords], double (&x)[6]) {
    double L[21];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const double ajj = S[icp_upper(j, j)];
        double d = ajj;
#pragma unroll
        for (int k = 0; k < j; ++k) d = d - L[icp_lower(j, k)] * L[icp_lower(j, k)];
        if (d <= 0x1p-40 * ajj || !std::isfinite(d)) ok = false;
        const double l = sqrt(d);
        L[icp_lower(j, j)] = l;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double s = S[icp_upper(j, i)];
#pragma unroll
            for (int k = 0; k < j; ++k) s = s - L[icp_lower(i, k)] * L[icp_lower(j, k)];
            L[icp_lower(i, j)] = s / l;
        }
    }
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double s = -S[21 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = s - L[icp_lower(i, k)] * y[k];
        y[i] = s / L[icp_lower(i, i)];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) s = s - L[icp_lower(k, i)] * x[k];
        x[i] = s / L[icp_lower(i, i)];
    }
    return ok;
}

__global__ __launch_bounds__(kThreads) void icp_finish_kernel(int tiles, int metric, int eval, double tol_rot, double tol_trans,
                                                              const double *__restrict__ partial, double *__restrict__ T,
                                                              double *__restrict__ sums, int64_t *__restrict__ count,
                                                              double *__restrict__ xout, int32_t *__restrict__ status,
                                                              int32_t *__restrict__ iters, int32_t *__restrict__ err) {
    __shared__ double s_chunk[kSumChunks][32];
    const int b = blockIdx.x;
    if (!eval && (status[b] & (PN2_ICP_CONVERGED | PN2_ICP_SINGULAR)) != 0) return;        // frozen: nothing is touched
    double S[kIcpWords];
    if (!pn2_tile_total(partial + (int64_t)b * tiles * kIcpWords, tiles, s_chunk, S)) return;
#pragma unroll
    for (int q = 0; q < kIcpSums; ++q) sums[(int64_t)b * kIcpSums + q] = S[q];
    const int64_t n = (int64_t)S[kIcpSums];
    count[b] = n;
    if (eval) return;

    double R[12];
    bool finite = true;
#pragma unroll
    for (int q = 0; q < 12; ++q) {
        R[q] = T[(int64_t)b * 12 + q];
        finite = finite && std::isfinite(R[q]);
    }
#pragma unroll
    for (int q = 0; q < kIcpSums; ++q) finite = finite && std::isfinite(S[q]);
    double x[6];
    const bool solved = icp_solve(S, x);
    const bool few = n < (metric == PN2_ICP_PLANE ? 6 : 3);
    if (!finite || few || !solved) {
#pragma unroll
        for (int q = 0; q < 6; ++q) xout[(int64_t)b * 6 + q] = 0.0;
        status[b] = status[b] | PN2_ICP_SINGULAR;
        if (err != nullptr) atomicOr(err, finite ? PN2_ICP_ERR_SINGULAR : PN2_ICP_ERR_NONFINITE);
        return;
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) xout[(int64_t)b * 6 + q] = x[q];
    const double w0 = x[0], w1 = x[1], w2 = x[2];
    const double th = sqrt((w0 * w0 + w1 * w1) + w2 * w2), tt = th * th;
    double a, bb;
    if (th < 0x1p-20) {
        a = 1.0 - tt / 6.0;
        bb = 0.5 - tt / 24.0;
    } else {
        a = sin(th) / th;
        bb = (1.0 - cos(th)) / tt;
    }
    const double K[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
    const double K2[9] = {-(w1 * w1 + w2 * w2), w0 * w1, w0 * w2, w0 * w1, -(w0 * w0 + w2 * w2), w1 * w2, w0 * w2, w1 * w2, -(w0 * w0 + w1 * w1)};
    double D[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) D[q] = ((q % 4 == 0 ? 1.0 : 0.0) + a * K[q]) + bb * K2[q];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) T[(int64_t)b * 12 + i * 4 + j] = (D[i * 3] * R[j] + D[i * 3 + 1] * R[4 + j]) + D[i * 3 + 2] * R[8 + j];
        T[(int64_t)b * 12 + i * 4 + 3] = ((D[i * 3] * R[3] + D[i * 3 + 1] * R[7]) + D[i * 3 + 2] * R[11]) + x[3 + i];
    }
    iters[b] = iters[b] + 1;
    const double step = sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]);
    if (th <= tol_rot && step <= tol_trans) status[b] = status[b] | PN2_ICP_CONVERGED;
}

}  // namespace

extern "C" {

int64_t pn2_icp_workspace_bytes(int B, int N) {
    return pn2_cloud_shape_ok(B, N) ? pn2_round16((int64_t)B * pn2_cdiv(N, kSumTile) * kIcpWords * (int64_t)sizeof(double)) : PN2_EINVAL;
}

int pn2_icp_step(const float *src, int lds, int B, int N, const int64_t *n_src, const float *tgt, int ldt, int M, const float *tgt_normal,
                 int ldn, const double *origin, const double *cell, const void *grid_workspace, float max_d2, int metric, int flags,
                 double tol_rot, double tol_trans, double *T, double *sums, int64_t *count, double *x, int32_t *status, int32_t *iters,
                 int64_t *corr, int32_t *err, void *workspace, pn2_stream_t stream) {
    PN2_CHECK_ARG(src && tgt && origin && cell && grid_workspace && T && sums && count && workspace);
    PN2_CHECK_ARG((flags & ~PN2_ICP_EVAL_ONLY) == 0 && (metric == PN2_ICP_POINT || metric == PN2_ICP_PLANE));
    const int eval = (flags & PN2_ICP_EVAL_ONLY) != 0;
    PN2_CHECK_ARG(eval || (x && status && iters));
    PN2_CHECK_ARG(pn2_cloud_shape_ok(B, N) && grid_shape_ok(B, M));
    PN2_CHECK_ARG(lds >= 3 && lds <= 16 && ldt >= 3 && ldt <= 16);
    PN2_CHECK_ARG(metric == PN2_ICP_POINT || (tgt_normal != nullptr && ldn >= 3 && ldn <= 16));
    PN2_CHECK_ARG(std::isfinite(tol_rot) && std::isfinite(tol_trans) && tol_rot >= 0.0 && tol_trans >= 0.0);
    PN2_CHECK_ARG(pn2_aligned(src, 4) && pn2_aligned(tgt, 4) && pn2_aligned(tgt_normal, 4) && pn2_aligned(grid_workspace, 16));
    PN2_CHECK_ARG(pn2_aligned(T, 8) && pn2_aligned(sums, 8) && pn2_aligned(count, 8) && pn2_aligned(x, 8) && pn2_aligned(corr, 8));
    PN2_CHECK_ARG(pn2_aligned(n_src, 8) && pn2_aligned(status, 4) && pn2_aligned(iters, 4) && pn2_aligned(err, 4) && pn2_aligned(workspace, 8));
    Grid grid;
    PN2_CHECK_ARG(pn2_grid_from(origin, cell, grid));
    const Work w = grid_work(B, M, const_cast<void *>(grid_workspace));         // (only read)
    const int tiles = (int)pn2_cdiv(N, kSumTile);
    double *partial = static_cast<double *>(workspace);
    const hipStream_t s = pn2_s(stream);
    const dim3 by_tile((unsigned)tiles, (unsigned)B);
    if (metric == PN2_ICP_PLANE)
        hipLaunchKernelGGL(icp_accumulate_kernel<PN2_ICP_PLANE>, by_tile, dim3(kThreads), 0, s, src, lds, N, n_src, tgt, ldt, M, tgt_normal, ldn,
                           grid, w, max_d2, eval, T, status, corr, err, partial);
    else
        hipLaunchKernelGGL(icp_accumulate_kernel<PN2_ICP_POINT>, by_tile, dim3(kThreads), 0, s, src, lds, N, n_src, tgt, ldt, M, tgt_normal, ldn,
                           grid, w, max_d2, eval, T, status, corr, err, partial);
    hipLaunchKernelGGL(icp_finish_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, tiles, metric, eval, tol_rot, tol_trans, partial, T, sums,
                       count, x, status, iters, err);
    return pn2_launch_status();
}

}  // extern "C"
