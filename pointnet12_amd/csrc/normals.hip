// Surface normals and local PCA over neighbour lists: pn2_local_pca (include/pn2.h, "local PCA").
//
// COMPILED WITH -ffp-contract=off: the covariance is the one-pass fp64 statement of the header, add by add and product by
// product (fp64 add, multiply and divide are correctly rounded), so `cov` equals its numpy statement bit for bit.
#include "pn2_common.h"
#include "sym_eig3.h"

namespace {

constexpr int PCA_THREADS = 256;
// slots whose index, distance and point loads are issued together before the first of them is accumulated (the chain
// idx -> point is two dependent misses; a compile-time constant, every array index below is one): make XFLAGS=-DPN2_PCA_UNROLL=n
#ifndef PN2_PCA_UNROLL
#define PN2_PCA_UNROLL 4
#endif

__device__ __forceinline__ bool pca_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }          // (false for NaN)

struct PcaSums {
    double s1x = 0.0, s1y = 0.0, s1z = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
    double p0x = 0.0, p0y = 0.0, p0z = 0.0;
    int cnt = 0;
    bool finite = true;
};

// U consecutive slots: their index and distance loads are issued together, then their candidate rows, then they are accumulated
// in slot order.  An invalid slot loads candidate 0 (in bounds) and is masked out of the sums.
template <int U, bool DIST>
__device__ __forceinline__ void pca_slots(PcaSums &a, const int64_t *__restrict__ ri, const float *__restrict__ rd,
                                          const float *__restrict__ c, int ldc, int M, float max_d2) {
    int64_t i[U];
    float d[U];
    bool ok[U];
    float px[U], py[U], pz[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
        i[j] = ri[j];
        d[j] = DIST ? rd[j] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < U; ++j) {
        ok[j] = (i[j] >= 0) & (i[j] < M) & !(DIST & (d[j] > max_d2));       // (no dist: no cut-off; a NaN distance is kept)
        const float *p = c + (size_t)(ok[j] ? i[j] : 0) * ldc;
        px[j] = p[0]; py[j] = p[1]; pz[j] = p[2];
    }
#pragma unroll
    for (int j = 0; j < U; ++j) {
        if (ok[j]) {
            const double x = (double)px[j], y = (double)py[j], z = (double)pz[j];
            a.finite = a.finite && pca_finite(px[j]) && pca_finite(py[j]) && pca_finite(pz[j]);
            if (a.cnt == 0) { a.p0x = x; a.p0y = y; a.p0z = z; }
            const double dx = x - a.p0x, dy = y - a.p0y, dz = z - a.p0z;
            a.s1x += dx; a.s1y += dy; a.s1z += dz;
            a.sxx += dx * dx; a.sxy += dx * dy; a.sxz += dx * dz;
            a.syy += dy * dy; a.syz += dy * dz; a.szz += dz * dz;
            ++a.cnt;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// One row per lane, nine fp64 accumulators, one pass over the row's K slots in ascending order; nothing is sized by K.  Each
// lane walks its own idx / dist row (8 K and 4 K contiguous bytes: the lane's cache lines are used whole over the K steps, and
// a tile staged through LDS would have to be transposed for every K); the candidate rows are random 12-byte reads.  No lane waits on
// another: no barrier, no shuffle.
// ---------------------------------------------------------------------------------------------
template <bool DIST>
__global__ __launch_bounds__(PCA_THREADS) void local_pca_kernel(const float *__restrict__ query, int ldq, const float *__restrict__ cand,
                                                                int ldc, const int64_t *__restrict__ idx, const float *__restrict__ dist,
                                                                int N, int M, int K, float max_d2, const int64_t *__restrict__ n_query,
                                                                const float *__restrict__ viewpoint, float *__restrict__ normal, int ldn,
                                                                float *__restrict__ eig, double *__restrict__ cov,
                                                                int32_t *__restrict__ count, int32_t *__restrict__ err) {
    const int b = blockIdx.y;
    const int n = blockIdx.x * PCA_THREADS + threadIdx.x;
    if (n >= pn2_rows_or_all(n_query, b, N)) return;
    const size_t row = (size_t)b * N + n;
    const int64_t *ri = idx + row * K;
    const float *rd = DIST ? dist + row * K : nullptr;
    const float *c = cand + (size_t)b * M * ldc;

    PcaSums a;
    int k = 0;
    for (; k + PN2_PCA_UNROLL <= K; k += PN2_PCA_UNROLL) pca_slots<PN2_PCA_UNROLL, DIST>(a, ri + k, DIST ? rd + k : nullptr, c, ldc, M, max_d2);
    for (; k < K; ++k) pca_slots<1, DIST>(a, ri + k, DIST ? rd + k : nullptr, c, ldc, M, max_d2);
    const int cnt = a.cnt;
    bool finite = a.finite;
    const double s1x = a.s1x, s1y = a.s1y, s1z = a.s1z, sxx = a.sxx, sxy = a.sxy, sxz = a.sxz, syy = a.syy, syz = a.syz, szz = a.szz;

    double vx = 0.0, vy = 0.0, vz = 0.0;                       // viewpoint - query
    if (viewpoint != nullptr) {
        const float *q = query + row * ldq;
        const float qx = q[0], qy = q[1], qz = q[2];
        finite = finite && pca_finite(qx) && pca_finite(qy) && pca_finite(qz);
        vx = (double)viewpoint[3 * b] - (double)qx;
        vy = (double)viewpoint[3 * b + 1] - (double)qy;
        vz = (double)viewpoint[3 * b + 2] - (double)qz;
    }

    double cxx = 0.0, cxy = 0.0, cxz = 0.0, cyy = 0.0, cyz = 0.0, czz = 0.0;
    if (cnt > 0) {
        const double dn = (double)cnt;
        const double mx = s1x / dn, my = s1y / dn, mz = s1z / dn;
        cxx = sxx / dn - mx * mx; cxy = sxy / dn - mx * my; cxz = sxz / dn - mx * mz;
        cyy = syy / dn - my * my; cyz = syz / dn - my * mz; czz = szz / dn - mz * mz;
    }
    double l0 = 0.0, l1 = 0.0, l2 = 0.0, ux = 0.0, uy = 0.0, uz = 0.0;
    if (finite) {
        pn2_sym_eig3(cxx, cxy, cxz, cyy, cyz, czz, l0, l1, l2, ux, uy, uz);
        l0 = l0 > 0.0 ? l0 : 0.0;                               // (a computed value below zero, and -0.0, become +0.0)
        l1 = l1 > 0.0 ? l1 : 0.0;
        l2 = l2 > 0.0 ? l2 : 0.0;
    }
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (finite && cnt >= 3) {
        const double s = viewpoint != nullptr ? (ux * vx + uy * vy) + uz * vz : 0.0;
        bool flip = s < 0.0;
        if (s == 0.0) flip = uz < 0.0 || (uz == 0.0 && (uy < 0.0 || (uy == 0.0 && ux < 0.0)));      // +z, then +y, then +x
        nx = (float)(flip ? -ux : ux);
        ny = (float)(flip ? -uy : uy);
        nz = (float)(flip ? -uz : uz);
    }
    float e0 = (float)l0, e1 = (float)l1, e2 = (float)l2;
    if (!finite) {
        const float qn = __uint_as_float(0x7FC00000u);
        const double qd = __longlong_as_double(0x7FF8000000000000LL);
        nx = ny = nz = e0 = e1 = e2 = qn;
        cxx = cxy = cxz = cyy = cyz = czz = qd;
    }
    if (normal != nullptr) {
        float *o = normal + row * ldn;
        o[0] = nx; o[1] = ny; o[2] = nz;
    }
    if (eig != nullptr) {
        float *o = eig + row * 3;
        o[0] = e0; o[1] = e1; o[2] = e2;
    }
    if (cov != nullptr) {
        double *o = cov + row * 6;
        o[0] = cxx; o[1] = cxy; o[2] = cxz; o[3] = cyy; o[4] = cyz; o[5] = czz;
    }
    if (count != nullptr) count[row] = cnt;
    const int flags = (!finite ? PN2_PCA_ERR_NONFINITE : 0) | ((finite && cnt < 3) ? PN2_PCA_ERR_FEW : 0);
    if (flags != 0 && err != nullptr) atomicOr(err, flags);
}

}  // namespace

extern "C" {

int pn2_local_pca(const float *query, int ldq, const float *cand, int ldc, const int64_t *idx, const float *dist, int B, int N, int M,
                  int K, float max_d2, const int64_t *n_query, const float *viewpoint, float *normal, int ldn, float *eig, double *cov,
                  int32_t *count, int32_t *err, pn2_stream_t stream) {
    PN2_CHECK_ARG(cand && idx && B > 0 && N > 0 && M > 0 && K >= 1 && B <= 65535 && N <= 0x7FFFFF00);
    PN2_CHECK_ARG(ldc >= 3 && ldc <= 16 && (viewpoint == nullptr || query != nullptr));
    PN2_CHECK_ARG(query == nullptr || (ldq >= 3 && ldq <= 16));
    PN2_CHECK_ARG(normal == nullptr || ldn >= 3);
    const dim3 grid((unsigned)pn2_cdiv(N, PCA_THREADS), B);
    if (dist != nullptr)
        hipLaunchKernelGGL(local_pca_kernel<true>, grid, dim3(PCA_THREADS), 0, pn2_s(stream), query, ldq, cand, ldc, idx, dist, N, M, K,
                           max_d2, n_query, viewpoint, normal, ldn, eig, cov, count, err);
    else
        hipLaunchKernelGGL(local_pca_kernel<false>, grid, dim3(PCA_THREADS), 0, pn2_s(stream), query, ldq, cand, ldc, idx, dist, N, M, K,
                           max_d2, n_query, viewpoint, normal, ldn, eig, cov, count, err);
    return pn2_launch_status();
}

}  // extern "C"
