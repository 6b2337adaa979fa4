// PointNetDenseCls (model/pointnet.py:153-228 of the reference, the part-segmentation net of partseg.py), ABI 13.
// Its convs1 is a 1x1 conv over a 4944-channel concatenation [out_max | label] * N ++ out1 ++ out2 ++ out3 ++ out4 ++ out5;
// the library never builds it:
//   - the per-cloud 2064 columns become one [B]-row GEMM (W_g g_b, pn2_conv1x1_fwd) added in the epilogue of
//   - the per-point 2880 columns: ONE GEMM whose operand is read from the five sources in place (pn2_conv1x1_fwd_multi and
//     pn2_conv1x1_wgrad_multi, mlp.hip, on the streamed-weight NT / TN cores with the LoadMulti operand of mlp_loaders.h).
//     out5 = bn5(conv5(.)) (no ReLU) is never stored: the loader applies bn5 to the saved pre-BN rows.
// Here: the data gradient into per-source outputs, and the backward reduction of bn5, whose output feeds both the max over the
// cloud (out_max) and convs1 (dense).
#include "mlp_host.h"

namespace {

// dZ[g K + k, c] = dDense[g K + k, c] + (k == arg[g, c] ? dPool[g, c] : 0); red += sum dZ, sum dZ * yhat (yhat = (y - mean) * invstd).
// A thread owns one column quad and walks the rows q, q + 4, ... of its workgroup's row range (group / position advanced
// incrementally: no division per row).  dDense may alias dZ (each element is read, then written, by the same thread).
__global__ __launch_bounds__(256) void bn_bwd_noact_dense_kernel(const float *dDense, int ldd, const float *__restrict__ dPool, int ldp,
                                                                 const int32_t *__restrict__ arg, int lda, const float *__restrict__ Y,
                                                                 int ldy, const float *__restrict__ aff, int ldf, int64_t P, int K, int C,
                                                                 int64_t rows_per_wg, float *dZ, int ldz, double *__restrict__ red) {
    __shared__ double sh[2][4][256];
    const int qi = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int cq = (blockIdx.x * 64 + qi) * 4;
    const int64_t p0 = (int64_t)blockIdx.y * rows_per_wg;
    const int64_t p1 = p0 + rows_per_wg < P ? p0 + rows_per_wg : P;
    double s0[4] = {0.0, 0.0, 0.0, 0.0}, s1[4] = {0.0, 0.0, 0.0, 0.0};
    if (cq < ldf) {
        Affine a(aff, ldf);
        const float4 mu = ld4(a.mean + cq), is = ld4(a.invstd + cq);
        const float mua[4] = {mu.x, mu.y, mu.z, mu.w}, isa[4] = {is.x, is.y, is.z, is.w};
        int64_t p = p0 + rl;
        int64_t g = p / K;
        int k = (int)(p - g * K);
        for (; p < p1; p += 4) {
            const float4 dd = ld4(dDense + p * ldd + cq), y = ld4(Y + p * ldy + cq);
            const float4 dp = ld4(dPool + g * ldp + cq);
            const int4 am = ld4i(arg + g * lda + cq);
            const float dda[4] = {dd.x, dd.y, dd.z, dd.w}, ya[4] = {y.x, y.y, y.z, y.w}, dpa[4] = {dp.x, dp.y, dp.z, dp.w};
            const int aa[4] = {am.x, am.y, am.z, am.w};
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v = dda[e] + (aa[e] == k ? dpa[e] : 0.f);
                o[e] = cq + e < C ? v : 0.f;
                s0[e] += (double)o[e];
                s1[e] += (double)(o[e] * ((ya[e] - mua[e]) * isa[e]));
            }
            *reinterpret_cast<float4 *>(dZ + p * ldz + cq) = make_float4(o[0], o[1], o[2], o[3]);
            k += 4;
            while (k >= K) { k -= K; ++g; }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { sh[0][rl][qi * 4 + e] = s0[e]; sh[1][rl][qi * 4 + e] = s1[e]; }
    __syncthreads();
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < C) {
        const int col = threadIdx.x;
        const double a0 = ((sh[0][0][col] + sh[0][1][col]) + sh[0][2][col]) + sh[0][3][col];
        const double a1 = ((sh[1][0][col] + sh[1][1][col]) + sh[1][2][col]) + sh[1][3][col];
        double *rep = red + (size_t)(blockIdx.y % PN2_STAT_REPLICAS) * 2 * C;
        atomicAdd(rep + c, a0);
        atomicAdd(rep + C + c, a1);
    }
}

}  // namespace

extern "C" {

// One launch of the existing data-gradient core per source, on the column window W[:, k_i : k_i + K_i] read in place.  (A single
// launch over a destination table would form dY once instead of nsrc times; at 16 x 2048 points and M = 256 that is 4 x 64 MB
// of extra reads against a 2880-deep product -- see DESIGN.md, ABI 13.)
int pn2_conv1x1_dgrad_multi(const float *dZ, int ldz, const float *Y, int ldy, const float *coef, const float *W, int ldw,
                            float *const *dX, const int *lddx, const int *K, int nsrc, int64_t P, int M, pn2_stream_t stream) {
    PN2_CHECK_ARG(dZ && Y && coef && W && dX && lddx && K && nsrc >= 1 && nsrc <= PN2_MULTI_MAX && P > 0 && P < (1LL << 31) && M > 0);
    PN2_CHECK_ARG(ldz % 4 == 0 && ldz >= round4(M) && ldy % 4 == 0 && ldy >= round4(M));
    int64_t k0 = 0;
    for (int i = 0; i < nsrc; ++i) {
        PN2_CHECK_ARG(dX[i] && K[i] > 0 && K[i] % 4 == 0 && lddx[i] % 4 == 0 && lddx[i] >= K[i]);
        k0 += K[i];
    }
    PN2_CHECK_ARG(ldw >= k0);
    k0 = 0;
    for (int i = 0; i < nsrc; ++i) {
        const int rc = pn2_conv1x1_dgrad(dZ, ldz, nullptr, 0, nullptr, 0, Y, ldy, coef, W + k0, ldw, nullptr, 0, nullptr, dX[i], lddx[i],
                                         nullptr, P, M, K[i], nullptr, stream);
        if (rc != PN2_OK) return rc;
        k0 += K[i];
    }
    return PN2_OK;
}

int pn2_bn_bwd_reduce_noact_dense(const float *dDense, int ldd, const float *dPool, int ldp, const int32_t *arg, int lda, const float *Y,
                                  int ldy, const float *affine, int64_t G, int K, int C, float *dZ, int ldz, double *red,
                                  pn2_stream_t stream) {
    PN2_CHECK_ARG(dDense && dPool && arg && Y && affine && dZ && red && G > 0 && K > 0 && C > 0 && G * (int64_t)K < (1LL << 31));
    const int ld = round4(C);
    PN2_CHECK_ARG(ldd % 4 == 0 && ldp % 4 == 0 && lda % 4 == 0 && ldy % 4 == 0 && ldz % 4 == 0);
    PN2_CHECK_ARG(ldd >= ld && ldp >= ld && lda >= ld && ldy >= ld && ldz >= ld);
    PN2_CHECK_ARG(dDense == dZ ? ldd == ldz : true);
    const int64_t P = G * K;
    const unsigned gx = (unsigned)pn2_cdiv(ld, 256);
    int64_t wgs = (int64_t)pn2_num_cus() * 4 / gx;
    if (wgs < 1) wgs = 1;
    int64_t rows = pn2_cdiv(P, wgs);
    if (rows < 64) rows = 64;
    const int64_t gy = pn2_cdiv(P, rows);
    hipLaunchKernelGGL(bn_bwd_noact_dense_kernel, dim3(gx, (unsigned)gy), dim3(256), 0, pn2_s(stream), dDense, ldd, dPool, ldp, arg, lda, Y,
                       ldy, affine, ld, P, K, C, rows, dZ, ldz, red);
    return pn2_launch_status();
}

}  // extern "C"
