// PointNet v1 pieces (model/pointnet.py of the reference) that the PointNet++ kernels do not cover (ABI 12):
//   - the per-cloud k x k transform of torch.bmm(x, trans) and its two gradients (STN3d / STNkd outputs applied to every point);
//   - max over the whole cloud of BatchNorm output WITHOUT a ReLU (PointNetEncoder: bn3(conv3(x)) then torch.max) and its backward;
//   - the broadcast-concat layer of PointNetSeg.conv1, factorised: y_p = W_p pointfeat_p + b + (W_g g_b), with the per-cloud term
//     added (plus the BatchNorm statistics) in a pass of its own after the per-point GEMM, and the per-cloud column sums of dY its
//     backward needs.
// Everything here streams rows: no MFMA, no fp32 atomics.  Sums that must be run-to-run identical (dT, the column sums) leave as
// per-workgroup slabs in caller scratch and are added in a fixed order by a second launch.
#include "pn2_common.h"
#include "bn_affine.h"
#include "mlp_loaders.h"

namespace {

constexpr int kTfRows = 256;        // rows of one dT / column-sum slab
constexpr int kTfMaxK = 128;

__device__ __forceinline__ int r4d(int c) { return (c + 3) & ~3; }

// kTrans = false: out[b N + n, j] = sum_i X[b N + n, i] T[b, i, j]      (the forward, torch.bmm(x, trans))
// kTrans = true:  out[b N + n, i] = sum_j X[b N + n, j] T[b, i, j]      (the data gradient, X = dOut)
// T_b sits in LDS as a zero-padded [kp, kp] matrix (kp = round4(k)); a thread owns one output quad of a row and walks the row's
// input quads in order: one fp32 fma chain per output element.
template <bool kTrans>
__global__ __launch_bounds__(256) void point_transform_kernel(const float *__restrict__ X, int ldx, const float *__restrict__ T, int N,
                                                              int k, float *__restrict__ out, int ldo) {
    extern __shared__ float sT[];
    const int kp = r4d(k), q = kp >> 2;
    const int b = blockIdx.y;
    const float *Tb = T + (size_t)b * k * k;
    for (int e = threadIdx.x; e < kp * kp; e += 256) {
        const int i = e / kp, j = e - (e / kp) * kp;
        float v = 0.f;
        if (i < k && j < k) v = kTrans ? Tb[j * k + i] : Tb[i * k + j];
        sT[e] = v;
    }
    __syncthreads();
    const int rp = 256 / q;                    // rows per pass
    const int jq = threadIdx.x % q, rl = threadIdx.x / q;
    if (rl >= rp) return;
    const int64_t n0 = (int64_t)blockIdx.x * kTfRows;
    const int64_t n1 = n0 + kTfRows < N ? n0 + kTfRows : N;
    for (int64_t n = n0 + rl; n < n1; n += rp) {
        const float *x = X + ((int64_t)b * N + n) * ldx;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int i = 0; i < kp; i += 4) {
            const float4 xv = ld4(x + i);
            const float4 t0 = *reinterpret_cast<const float4 *>(sT + (i + 0) * kp + 4 * jq);
            const float4 t1 = *reinterpret_cast<const float4 *>(sT + (i + 1) * kp + 4 * jq);
            const float4 t2 = *reinterpret_cast<const float4 *>(sT + (i + 2) * kp + 4 * jq);
            const float4 t3 = *reinterpret_cast<const float4 *>(sT + (i + 3) * kp + 4 * jq);
            acc.x = __builtin_fmaf(xv.x, t0.x, acc.x); acc.y = __builtin_fmaf(xv.x, t0.y, acc.y);
            acc.z = __builtin_fmaf(xv.x, t0.z, acc.z); acc.w = __builtin_fmaf(xv.x, t0.w, acc.w);
            acc.x = __builtin_fmaf(xv.y, t1.x, acc.x); acc.y = __builtin_fmaf(xv.y, t1.y, acc.y);
            acc.z = __builtin_fmaf(xv.y, t1.z, acc.z); acc.w = __builtin_fmaf(xv.y, t1.w, acc.w);
            acc.x = __builtin_fmaf(xv.z, t2.x, acc.x); acc.y = __builtin_fmaf(xv.z, t2.y, acc.y);
            acc.z = __builtin_fmaf(xv.z, t2.z, acc.z); acc.w = __builtin_fmaf(xv.z, t2.w, acc.w);
            acc.x = __builtin_fmaf(xv.w, t3.x, acc.x); acc.y = __builtin_fmaf(xv.w, t3.y, acc.y);
            acc.z = __builtin_fmaf(xv.w, t3.z, acc.z); acc.w = __builtin_fmaf(xv.w, t3.w, acc.w);
        }
        *reinterpret_cast<float4 *>(out + ((int64_t)b * N + n) * ldo + 4 * jq) = acc;
    }
}

__device__ __forceinline__ void outer4(float (&acc)[16], const float4 x, const float4 d) {
    const float xa[4] = {x.x, x.y, x.z, x.w}, da[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a * 4 + c] = __builtin_fmaf(xa[a], da[c], acc[a * 4 + c]);
}

// part[(b nch + ch) k k + i k + j] = sum over the rows n of slab ch of X[b N + n, i] D[b N + n, j].  A thread owns 4 x 4 output
// blocks; where there are fewer than 256 blocks (k < 64) the rows of the slab are dealt to 256 / blocks lanes whose partial blocks
// are added in lane order through LDS.
__global__ __launch_bounds__(256) void point_transform_dt_part_kernel(const float *__restrict__ X, int ldx, const float *__restrict__ D,
                                                                      int ldd, int N, int k, float *__restrict__ part) {
    __shared__ float red[256 * 16];
    const int kp = r4d(k), q = kp >> 2, nblk = q * q;
    const int b = blockIdx.y, ch = blockIdx.x, nch = gridDim.x;
    const int64_t n0 = (int64_t)ch * kTfRows;
    const int64_t n1 = n0 + kTfRows < N ? n0 + kTfRows : N;
    const float *Xb = X + (int64_t)b * N * ldx, *Db = D + (int64_t)b * N * ldd;
    float *dst = part + ((size_t)b * nch + ch) * k * k;
    const int t = threadIdx.x;
    if (nblk >= 256) {
        for (int bi = t; bi < nblk; bi += 256) {
            const int iq = bi / q, jq = bi - (bi / q) * q;
            float acc[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.f;
            for (int64_t n = n0; n < n1; ++n) outer4(acc, ld4(Xb + n * ldx + 4 * iq), ld4(Db + n * ldd + 4 * jq));
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int i = 4 * iq + a, j = 4 * jq + c;
                    if (i < k && j < k) dst[i * k + j] = acc[a * 4 + c];
                }
        }
        return;
    }
    const int lanes = 256 / nblk;
    const int bi = t % nblk, lane = t / nblk;
    const int iq = bi / q, jq = bi - (bi / q) * q;
    float acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    if (lane < lanes)
        for (int64_t n = n0 + lane; n < n1; n += lanes) outer4(acc, ld4(Xb + n * ldx + 4 * iq), ld4(Db + n * ldd + 4 * jq));
    if (lane < lanes) {
#pragma unroll
        for (int e = 0; e < 16; ++e) red[(lane * nblk + bi) * 16 + e] = acc[e];
    }
    __syncthreads();
    if (t < nblk) {
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = red[t * 16 + e];
        for (int l = 1; l < lanes; ++l) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] += red[(l * nblk + t) * 16 + e];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int i = 4 * iq + a, j = 4 * jq + c;
                if (i < k && j < k) dst[i * k + j] = acc[a * 4 + c];
            }
    }
}

// dst[g, e] = sum over the nch slabs of part[(g nch + ch) * len + e], in slab order.
__global__ __launch_bounds__(256) void slab_sum_kernel(const float *__restrict__ part, int nch, int len, float *__restrict__ dst, int ldd,
                                                       int len_pad) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int g = blockIdx.y;
    if (e >= len_pad) return;
    float s = 0.f;
    if (e < len) {
        const float *p = part + (size_t)g * nch * len + e;
        for (int ch = 0; ch < nch; ++ch) s += p[(size_t)ch * len];
    }
    dst[(size_t)g * ldd + e] = s;
}

// out[g, c] = max_k bn(Y[g K + k, c]) (no ReLU), arg[g, c] = first k attaining it.  A workgroup owns 16 channels (four quads) of
// one group; 64 row lanes per quad each keep the (max, first k) of the rows they visit in ascending order (strict >), and the
// lanes are folded in lane order with "greater, or equal and smaller k" -- the tie rule of pn2_bn_relu_max.  A channel whose scale
// is 0 gives beta on every row and names row 0.
__global__ __launch_bounds__(256) void bn_max_kernel(const float *__restrict__ Y, int ldy, const float *__restrict__ aff, int lda, int64_t G,
                                                     int K, float *__restrict__ out, int ldo, int32_t *__restrict__ arg) {
    __shared__ float sv[64][16];
    __shared__ int sk[64][16];
    const int qi = threadIdx.x & 3, lane = threadIdx.x >> 2;
    const int cq = (blockIdx.x * 4 + qi) * 4;
    const bool colv = cq < lda;
    Affine a(aff, lda);
    float4 mu = make_float4(0.f, 0.f, 0.f, 0.f), sc = mu, be = mu;
    if (colv) { mu = ld4(a.mean + cq); sc = ld4(a.scale + cq); be = ld4(a.beta + cq); }
    for (int64_t g = blockIdx.y; g < G; g += gridDim.y) {
        float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        int bk[4] = {0, 0, 0, 0};
        if (colv) {
            const float *y = Y + g * K * ldy + cq;
            for (int k = lane; k < K; k += 64) {
                const float4 v = ld4(y + (int64_t)k * ldy);
                const float o[4] = {bn_act(v.x, mu.x, sc.x, be.x), bn_act(v.y, mu.y, sc.y, be.y), bn_act(v.z, mu.z, sc.z, be.z),
                                    bn_act(v.w, mu.w, sc.w, be.w)};
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (o[e] > best[e]) { best[e] = o[e]; bk[e] = k; }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) { sv[lane][qi * 4 + e] = best[e]; sk[lane][qi * 4 + e] = bk[e]; }
        __syncthreads();
        if (threadIdx.x < 16) {
            const int col = threadIdx.x;
            float bv = sv[0][col];
            int bkk = sk[0][col];
            for (int l = 1; l < 64; ++l) {
                const float ov = sv[l][col];
                const int ok = sk[l][col];
                if (ov > bv || (ov == bv && ok < bkk)) { bv = ov; bkk = ok; }
            }
            const int c = blockIdx.x * 16 + col;
            if (c < lda) {
                out[g * ldo + c] = bv;
                if (arg) arg[g * ldo + c] = bkk;
            }
        }
        __syncthreads();
    }
}

// dZp[g, c] = dOut[g, c] (pad lanes 0); red[c] += sum_g dOut, red[C + c] += sum_g dOut * yhat(Y[g K + arg, c]).
__global__ __launch_bounds__(256) void pool_bwd_noact_kernel(const float *__restrict__ dOut, int ldg, const int32_t *__restrict__ arg,
                                                             int ldo, const float *__restrict__ Y, int ldy, const float *__restrict__ aff,
                                                             int lda, int64_t G, int K, int C, float *__restrict__ dZp,
                                                             double *__restrict__ red) {
    __shared__ double sh[2][4][64];
    const int cl = threadIdx.x & 63, gl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    double s0 = 0.0, s1 = 0.0;
    if (c < lda) {
        Affine a(aff, lda);
        const bool real = c < C;
        const float mu = real ? a.mean[c] : 0.f, is = real ? a.invstd[c] : 0.f;
        for (int64_t g = (int64_t)blockIdx.y * 4 + gl; g < G; g += (int64_t)gridDim.y * 4) {
            const float dz = real ? dOut[g * ldg + c] : 0.f;
            dZp[g * ldo + c] = dz;
            if (real) {
                const float y = Y[(g * K + arg[g * ldo + c]) * ldy + c];
                s0 += (double)dz;
                s1 += (double)(dz * ((y - mu) * is));
            }
        }
    }
    sh[0][gl][cl] = s0; sh[1][gl][cl] = s1;
    __syncthreads();
    if (gl == 0 && c < C) {
        const double a0 = sh[0][0][cl] + sh[0][1][cl] + sh[0][2][cl] + sh[0][3][cl];
        const double a1 = sh[1][0][cl] + sh[1][1][cl] + sh[1][2][cl] + sh[1][3][cl];
        double *rep = red + (size_t)(blockIdx.y % PN2_STAT_REPLICAS) * 2 * C;
        atomicAdd(rep + c, a0);
        atomicAdd(rep + C + c, a1);
    }
}

// Y[p, c] += gbias[(p / rpg), c] in place; stats (may be NULL) += sum y, sum y^2 of the result per channel.
__global__ __launch_bounds__(256) void add_gbias_kernel(float *__restrict__ Y, int ldy, const float *__restrict__ gb, int ldg, int64_t rpg,
                                                        int64_t P, int N, int64_t rows_per_wg, double *__restrict__ stats) {
    __shared__ double sh[2][4][256];
    const int qi = threadIdx.x & 63, lane = threadIdx.x >> 6;
    const int cq = (blockIdx.x * 64 + qi) * 4;
    const int ld = r4d(N);
    const int64_t p0 = (int64_t)blockIdx.y * rows_per_wg;
    const int64_t p1 = p0 + rows_per_wg < P ? p0 + rows_per_wg : P;
    double s0[4] = {0.0, 0.0, 0.0, 0.0}, s1[4] = {0.0, 0.0, 0.0, 0.0};
    if (cq < ld) {
        for (int64_t p = p0 + lane; p < p1; p += 4) {
            float4 y = ld4(Y + p * ldy + cq);
            const float *g = gb + (p / rpg) * ldg + cq;
            float o[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (cq + e < N) o[e] += g[e];
                s0[e] += (double)o[e];
                s1[e] += (double)o[e] * (double)o[e];
            }
            *reinterpret_cast<float4 *>(Y + p * ldy + cq) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
    if (stats == nullptr) return;
#pragma unroll
    for (int e = 0; e < 4; ++e) { sh[0][lane][qi * 4 + e] = s0[e]; sh[1][lane][qi * 4 + e] = s1[e]; }
    __syncthreads();
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < N) {
        const int col = threadIdx.x;
        const double a0 = sh[0][0][col] + sh[0][1][col] + sh[0][2][col] + sh[0][3][col];
        const double a1 = sh[1][0][col] + sh[1][1][col] + sh[1][2][col] + sh[1][3][col];
        double *rep = stats + (size_t)(blockIdx.y % PN2_STAT_REPLICAS) * 2 * N;
        atomicAdd(rep + c, a0);
        atomicAdd(rep + N + c, a1);
    }
}

// part[(g nch + ch) * ld + c] = sum over the rows of slab ch of group g of dY = c0 dZ + q1 (y - mean) + q0.
__global__ __launch_bounds__(256) void colsum_part_kernel(const float *__restrict__ dZ, int ldz, const float *__restrict__ Y, int ldy,
                                                          const float *__restrict__ coef, int64_t rpg, int C, float *__restrict__ part) {
    __shared__ float sh[4][256];
    const int qi = threadIdx.x & 63, lane = threadIdx.x >> 6;
    const int ld = r4d(C);
    const int cq = (blockIdx.x * 64 + qi) * 4;
    const int64_t g = blockIdx.z, ch = blockIdx.y, nch = gridDim.y;
    const int64_t r0 = ch * kTfRows;
    const int64_t r1 = r0 + kTfRows < rpg ? r0 + kTfRows : rpg;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if (cq < ld) {
        const float4 c0 = ld4(coef + cq), q1 = ld4(coef + ld + cq), q0 = ld4(coef + 2 * ld + cq), mu = ld4(coef + 3 * ld + cq);
        const float c0a[4] = {c0.x, c0.y, c0.z, c0.w}, q1a[4] = {q1.x, q1.y, q1.z, q1.w}, q0a[4] = {q0.x, q0.y, q0.z, q0.w},
                    mua[4] = {mu.x, mu.y, mu.z, mu.w};
        for (int64_t r = r0 + lane; r < r1; r += 4) {
            const int64_t p = g * rpg + r;
            const float4 dz = ld4(dZ + p * ldz + cq), y = ld4(Y + p * ldy + cq);
            const float dza[4] = {dz.x, dz.y, dz.z, dz.w}, ya[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] += __builtin_fmaf(c0a[e], dza[e], __builtin_fmaf(q1a[e], ya[e] - mua[e], q0a[e]));
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) sh[lane][qi * 4 + e] = s[e];
    __syncthreads();
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < ld) {                                // (pad columns: zero coefficients give 0)
        const int col = threadIdx.x;
        part[(g * nch + ch) * ld + c] = ((sh[0][col] + sh[1][col]) + sh[2][col]) + sh[3][col];
    }
}

}  // namespace

extern "C" {

int64_t pn2_point_transform_workspace_bytes(int B, int N, int k) {
    if (B <= 0 || N <= 0 || k <= 0 || k > kTfMaxK) return 0;
    return (int64_t)B * pn2_cdiv(N, kTfRows) * k * k * (int64_t)sizeof(float);
}

int pn2_point_transform(const float *X, int ldx, const float *T, int B, int N, int k, float *out, int ldo, pn2_stream_t stream) {
    PN2_CHECK_ARG(X && T && out && B > 0 && B <= 65535 && N > 0 && k > 0 && k <= kTfMaxK);
    const int kp = (k + 3) & ~3;
    PN2_CHECK_ARG(ldx % 4 == 0 && ldo % 4 == 0 && ldx >= kp && ldo >= kp);
    hipLaunchKernelGGL(point_transform_kernel<false>, dim3((unsigned)pn2_cdiv(N, kTfRows), (unsigned)B), dim3(256),
                       (size_t)kp * kp * sizeof(float), pn2_s(stream), X, ldx, T, N, k, out, ldo);
    return pn2_launch_status();
}

int pn2_point_transform_bwd(const float *dOut, int ldd, const float *X, int ldx, const float *T, int B, int N, int k, float *dX, int lddx,
                            float *dT, void *workspace, pn2_stream_t stream) {
    PN2_CHECK_ARG(dOut && T && B > 0 && B <= 65535 && N > 0 && k > 0 && k <= kTfMaxK && (dX || dT));
    const int kp = (k + 3) & ~3;
    PN2_CHECK_ARG(ldd % 4 == 0 && ldd >= kp);
    PN2_CHECK_ARG(dX == nullptr || (lddx % 4 == 0 && lddx >= kp));              // (every refusal before the first launch)
    PN2_CHECK_ARG(dT == nullptr || (X && workspace && ldx % 4 == 0 && ldx >= kp));
    if (dX) {
        hipLaunchKernelGGL(point_transform_kernel<true>, dim3((unsigned)pn2_cdiv(N, kTfRows), (unsigned)B), dim3(256),
                           (size_t)kp * kp * sizeof(float), pn2_s(stream), dOut, ldd, T, N, k, dX, lddx);
        const int rc = pn2_launch_status();
        if (rc != PN2_OK) return rc;
    }
    if (dT) {
        const int nch = (int)pn2_cdiv(N, kTfRows);
        float *part = static_cast<float *>(workspace);
        hipLaunchKernelGGL(point_transform_dt_part_kernel, dim3((unsigned)nch, (unsigned)B), dim3(256), 0, pn2_s(stream), X, ldx, dOut, ldd,
                           N, k, part);
        hipLaunchKernelGGL(slab_sum_kernel, dim3((unsigned)pn2_cdiv(k * k, 256), (unsigned)B), dim3(256), 0, pn2_s(stream), part, nch,
                           k * k, dT, k * k, k * k);
    }
    return pn2_launch_status();
}

int pn2_bn_max(const float *Y, int ldy, const float *affine, int64_t G, int K, int C, float *out, int ldo, int32_t *arg,
               pn2_stream_t stream) {
    PN2_CHECK_ARG(Y && affine && out && G > 0 && K > 0 && C > 0);
    const int ld = (C + 3) & ~3;
    PN2_CHECK_ARG(ldy % 4 == 0 && ldo % 4 == 0 && ldy >= ld && ldo >= ld);
    const int64_t gy = G < 65535 ? G : 65535;
    hipLaunchKernelGGL(bn_max_kernel, dim3((unsigned)pn2_cdiv(ld, 16), (unsigned)gy), dim3(256), 0, pn2_s(stream), Y, ldy, affine, ld, G, K,
                       out, ldo, arg);
    return pn2_launch_status();
}

int pn2_pool_bwd_reduce_noact(const float *dOut, int ld_dout, const int32_t *arg, int ldo, const float *Y, int ldy, const float *affine,
                              int64_t G, int K, int C, float *dZp, double *red, pn2_stream_t stream) {
    PN2_CHECK_ARG(dOut && arg && Y && affine && dZp && red && G > 0 && K > 0 && C > 0 && ldo >= ((C + 3) & ~3) && ld_dout >= C &&
                  ldy >= C);
    int64_t gy = pn2_cdiv(G, 4);
    if (gy > 1024) gy = 1024;
    hipLaunchKernelGGL(pool_bwd_noact_kernel, dim3((unsigned)pn2_cdiv((C + 3) & ~3, 64), (unsigned)gy), dim3(256), 0, pn2_s(stream), dOut,
                       ld_dout, arg, ldo, Y, ldy, affine, (C + 3) & ~3, G, K, C, dZp, red);
    return pn2_launch_status();
}

int pn2_conv1x1_fwd_gbias(const float *X, int ldx, const float *W, int ldw, const float *bias, const float *gbias, int ldg,
                          int64_t rows_per_group, float *Y, int ldy, int64_t P, int K, int N, double *stats, pn2_stream_t stream) {
    PN2_CHECK_ARG(X && W && bias && gbias && Y && P > 0 && K > 0 && N > 0 && rows_per_group > 0 && P % rows_per_group == 0);
    PN2_CHECK_ARG(ldg >= N && ldy % 4 == 0 && ldy >= ((N + 3) & ~3));
    int rc = pn2_conv1x1_fwd(X, ldx, nullptr, W, ldw, bias, Y, ldy, P, K, N, nullptr, nullptr, stream);
    if (rc != PN2_OK) return rc;
    const unsigned gx = (unsigned)pn2_cdiv((N + 3) & ~3, 256);
    int64_t wgs = (int64_t)pn2_num_cus() * 4 / gx;
    if (wgs < 1) wgs = 1;
    int64_t rows = pn2_cdiv(P, wgs);
    if (rows < 16) rows = 16;
    const int64_t gy = pn2_cdiv(P, rows);
    hipLaunchKernelGGL(add_gbias_kernel, dim3(gx, (unsigned)gy), dim3(256), 0, pn2_s(stream), Y, ldy, gbias, ldg, rows_per_group, P, N,
                       rows, stats);
    return pn2_launch_status();
}

int64_t pn2_group_colsum_workspace_bytes(int64_t P, int64_t rows_per_group, int C) {
    if (P <= 0 || rows_per_group <= 0 || C <= 0 || P % rows_per_group) return 0;
    return (P / rows_per_group) * pn2_cdiv(rows_per_group, kTfRows) * ((C + 3) & ~3) * (int64_t)sizeof(float);
}

int pn2_group_colsum(const float *dZ, int ldz, const float *Y, int ldy, const float *coef, int64_t P, int64_t rows_per_group, int C,
                     float *s, int lds, void *workspace, pn2_stream_t stream) {
    PN2_CHECK_ARG(dZ && Y && coef && s && workspace && P > 0 && C > 0 && rows_per_group > 0 && P % rows_per_group == 0);
    const int ld = (C + 3) & ~3;
    PN2_CHECK_ARG(ldz % 4 == 0 && ldy % 4 == 0 && ldz >= ld && ldy >= ld && lds >= C);
    const int64_t G = P / rows_per_group;
    PN2_CHECK_ARG(G <= 65535);
    const int nch = (int)pn2_cdiv(rows_per_group, kTfRows);
    PN2_CHECK_ARG(nch <= 65535);
    float *part = static_cast<float *>(workspace);
    hipLaunchKernelGGL(colsum_part_kernel, dim3((unsigned)pn2_cdiv(ld, 256), (unsigned)nch, (unsigned)G), dim3(256), 0, pn2_s(stream), dZ,
                       ldz, Y, ldy, coef, rows_per_group, C, part);
    hipLaunchKernelGGL(slab_sum_kernel, dim3((unsigned)pn2_cdiv(lds < ld ? lds : ld, 256), (unsigned)G), dim3(256), 0, pn2_s(stream), part,
                       nch, ld, s, lds, lds < ld ? lds : ld);
    return pn2_launch_status();
}

}  // extern "C"
