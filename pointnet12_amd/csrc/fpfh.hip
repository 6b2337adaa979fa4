// FPFH point descriptors over neighbour lists: pn2_spfh (the integer pass) and pn2_fpfh (the weighted pass), include/pn2.h, "FPFH".
//
// COMPILED WITH -ffp-contract=off: the pair features and the weighted sum are the fp64 statement of the header, operation by
// operation (fp64 add, multiply, divide and square root are correctly rounded), so only atan2 may differ from a host libm, by a
// few ulp, and that only moves a pair whose t1 lies within 1e-15 of a bin edge.
#include "pn2_common.h"

namespace {

constexpr int FPFH_THREADS = 256;
constexpr int SPFH_WORDS = 9;                                    // 36 bytes a row: 33 counts, m, two zero bytes
constexpr double FPFH_PI = 3.14159265358979323846;

__device__ __forceinline__ bool fpfh_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }          // (false for NaN)
__device__ __forceinline__ bool fpfh_finite3(float x, float y, float z) { return fpfh_finite(x) && fpfh_finite(y) && fpfh_finite(z); }

__device__ __forceinline__ double fpfh_dot(double ax, double ay, double az, double bx, double by, double bz) {
    return (ax * bx + ay * by) + az * bz;
}

// floor(t) clamped to 0 .. 10 (a NaN goes to 0)
__device__ __forceinline__ int fpfh_bin(double t) { return !(t >= 1.0) ? 0 : (t >= 10.0 ? 10 : (int)t); }

// ---------------------------------------------------------------------------------------------
// pn2_spfh: one row per lane, slots in a loop, the row's point and normal in registers.  The 33 counters are indexed by a bin known
// only at run time: as a register array they would live in scratch.  They live in LDS instead, lane-private, four byte counters to
// a dword (a count is at most K <= 32: no carry), nine dwords a lane laid out word[w * blockDim + lane]: whatever w each lane
// picks, lane l's dword lies on bank l (mod 32 for the 32-bit accesses used here, which conflict inside a half-wave only).  Only the owning lane reads and writes its words (a plain read-modify-write:
// no LDS atomics, no barrier).  The loop is a three-stage rotation: while slot s is worked on, the point and the normal of slot
// s + 1 and the index of slot s + 2 are in flight (idx -> row is two dependent misses).  An invalid slot loads row 0, in bounds.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FPFH_THREADS) void spfh_kernel(const float *__restrict__ points, int ldp, const float *__restrict__ normals,
                                                            int ldn, const int64_t *__restrict__ idx, int M, int K, double max_d2,
                                                            const int64_t *__restrict__ n_points, uint32_t *__restrict__ out,
                                                            int32_t *__restrict__ err) {
    __shared__ uint32_t word[SPFH_WORDS * FPFH_THREADS];
    const int b = blockIdx.y;
    const int lane = threadIdx.x;
    const int i = blockIdx.x * FPFH_THREADS + lane;
    const int n = pn2_rows_or_all(n_points, b, M);
    if (i >= n) return;                                           // (no barrier below)
    const size_t row = (size_t)b * M + i;
    const int64_t *ri = idx + row * K;
    const float *P = points + (size_t)b * M * ldp;
    const float *Nn = normals + (size_t)b * M * ldn;
#pragma unroll
    for (int w = 0; w < SPFH_WORDS; ++w) word[w * FPFH_THREADS + lane] = 0u;

    const float pix = P[(size_t)i * ldp], piy = P[(size_t)i * ldp + 1], piz = P[(size_t)i * ldp + 2];
    const float nix = Nn[(size_t)i * ldn], niy = Nn[(size_t)i * ldn + 1], niz = Nn[(size_t)i * ldn + 2];
    const bool ni_finite = fpfh_finite3(nix, niy, niz);
    const bool ni_zero = nix == 0.f && niy == 0.f && niz == 0.f;

    int m = 0;
    bool nonfinite = false;
    int64_t j = ri[0];
    bool ok = j >= 0 && j < n;
    int64_t j_next = ri[K > 1 ? 1 : 0];
    const float *q = P + (size_t)(ok ? j : 0) * ldp, *qn = Nn + (size_t)(ok ? j : 0) * ldn;
    float pjx = q[0], pjy = q[1], pjz = q[2], njx = qn[0], njy = qn[1], njz = qn[2];
#pragma unroll 1
    for (int s = 0; s < K; ++s) {
        const bool ok_next = s + 1 < K && j_next >= 0 && j_next < n;
        const float *q1 = P + (size_t)(ok_next ? j_next : 0) * ldp, *qn1 = Nn + (size_t)(ok_next ? j_next : 0) * ldn;
        const float pkx = q1[0], pky = q1[1], pkz = q1[2], nkx = qn1[0], nky = qn1[1], nkz = qn1[2];
        const int64_t j_next2 = ri[s + 2 < K ? s + 2 : K - 1];
        if (ok) {
            double dx = (double)pjx - (double)pix, dy = (double)pjy - (double)piy, dz = (double)pjz - (double)piz;
            if (!(fpfh_finite3(pjx, pjy, pjz) && fpfh_finite3(pix, piy, piz))) {
                nonfinite = true;
            } else {
                const double d2 = fpfh_dot(dx, dy, dz, dx, dy, dz);
                if (d2 > 0.0 && d2 <= max_d2) {
                    const bool nj_finite = fpfh_finite3(njx, njy, njz);
                    const bool nj_zero = njx == 0.f && njy == 0.f && njz == 0.f;
                    if (!(ni_finite && nj_finite)) {
                        nonfinite = true;
                    } else if (!ni_zero && !nj_zero) {
                        const double d = sqrt(d2);
                        const double a1 = fpfh_dot((double)nix, (double)niy, (double)niz, dx, dy, dz) / d;
                        const double a2 = fpfh_dot((double)njx, (double)njy, (double)njz, dx, dy, dz) / d;
                        const bool on_j = fabs(a1) < fabs(a2);
                        const double sx = on_j ? (double)njx : (double)nix, sy = on_j ? (double)njy : (double)niy,
                                     sz = on_j ? (double)njz : (double)niz;
                        const double tx = on_j ? (double)nix : (double)njx, ty = on_j ? (double)niy : (double)njy,
                                     tz = on_j ? (double)niz : (double)njz;
                        const double f3 = on_j ? -a2 : a1;
                        if (on_j) { dx = -dx; dy = -dy; dz = -dz; }
                        double vx = dy * sz - dz * sy, vy = dz * sx - dx * sz, vz = dx * sy - dy * sx;
                        const double vl = sqrt(fpfh_dot(vx, vy, vz, vx, vy, vz));
                        if (vl > 0.0) {
                            vx = vx / vl; vy = vy / vl; vz = vz / vl;
                            const double wx = sy * vz - sz * vy, wy = sz * vx - sx * vz, wz = sx * vy - sy * vx;
                            const double f2 = fpfh_dot(vx, vy, vz, tx, ty, tz);
                            const double f1 = atan2(fpfh_dot(wx, wy, wz, tx, ty, tz) + 0.0, fpfh_dot(sx, sy, sz, tx, ty, tz));
                            const int b1 = fpfh_bin(11.0 * (f1 + FPFH_PI) / (2.0 * FPFH_PI));
                            const int b2 = 11 + fpfh_bin(11.0 * (f2 + 1.0) * 0.5);
                            const int b3 = 22 + fpfh_bin(11.0 * (f3 + 1.0) * 0.5);
                            word[(b1 >> 2) * FPFH_THREADS + lane] += 1u << ((b1 & 3) * 8);
                            word[(b2 >> 2) * FPFH_THREADS + lane] += 1u << ((b2 & 3) * 8);
                            word[(b3 >> 2) * FPFH_THREADS + lane] += 1u << ((b3 & 3) * 8);
                            ++m;
                        }
                    }
                }
            }
        }
        j = j_next; ok = ok_next; j_next = j_next2;
        pjx = pkx; pjy = pky; pjz = pkz; njx = nkx; njy = nky; njz = nkz;
    }
    uint32_t *o = out + row * SPFH_WORDS;
#pragma unroll
    for (int w = 0; w < SPFH_WORDS - 1; ++w) o[w] = word[w * FPFH_THREADS + lane];
    o[SPFH_WORDS - 1] = word[(SPFH_WORDS - 1) * FPFH_THREADS + lane] | ((uint32_t)m << 8);             // byte 32: the last count; byte 33: m
    const int flags = (m == 0 ? PN2_FPFH_ERR_EMPTY : 0) | (nonfinite ? PN2_FPFH_ERR_NONFINITE : 0);
    if (flags != 0 && err != nullptr) atomicOr(err, flags);
}

struct SpfhRow {
    uint32_t w[SPFH_WORDS];
};

__device__ __forceinline__ SpfhRow spfh_load(const uint32_t *__restrict__ p) {
    SpfhRow r;
#pragma unroll
    for (int k = 0; k < SPFH_WORDS; ++k) r.w[k] = p[k];
    return r;
}

// ---------------------------------------------------------------------------------------------
// pn2_fpfh: one row per lane, 33 fp64 accumulators plus W in registers, every index a compile-time constant.  A voting slot gathers
// the neighbour's nine dwords and its point; the same rotation as above keeps the next slot's in flight.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FPFH_THREADS) void fpfh_kernel(const float *__restrict__ points, int ldp, const int64_t *__restrict__ idx,
                                                            const uint32_t *__restrict__ spfh, int M, int K, double max_d2,
                                                            const int64_t *__restrict__ n_points, float *__restrict__ out,
                                                            int32_t *__restrict__ err) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * FPFH_THREADS + threadIdx.x;
    const int n = pn2_rows_or_all(n_points, b, M);
    if (i >= n) return;
    const size_t row = (size_t)b * M + i;
    const int64_t *ri = idx + row * K;
    const float *P = points + (size_t)b * M * ldp;
    const uint32_t *S = spfh + (size_t)b * M * SPFH_WORDS;
    const float pix = P[(size_t)i * ldp], piy = P[(size_t)i * ldp + 1], piz = P[(size_t)i * ldp + 2];
    const bool pi_finite = fpfh_finite3(pix, piy, piz);
    const SpfhRow own = spfh_load(S + (size_t)i * SPFH_WORDS);

    double A[33];
#pragma unroll
    for (int k = 0; k < 33; ++k) A[k] = 0.0;
    double W = 0.0;
    bool nonfinite = false;
    int64_t j = ri[0];
    bool ok = j >= 0 && j < n;
    int64_t j_next = ri[K > 1 ? 1 : 0];
    const float *q = P + (size_t)(ok ? j : 0) * ldp;
    float pjx = q[0], pjy = q[1], pjz = q[2];
    SpfhRow cur = spfh_load(S + (size_t)(ok ? j : 0) * SPFH_WORDS);
#pragma unroll 1
    for (int s = 0; s < K; ++s) {
        const bool ok_next = s + 1 < K && j_next >= 0 && j_next < n;
        const float *q1 = P + (size_t)(ok_next ? j_next : 0) * ldp;
        const float pkx = q1[0], pky = q1[1], pkz = q1[2];
        const SpfhRow nxt = spfh_load(S + (size_t)(ok_next ? j_next : 0) * SPFH_WORDS);
        const int64_t j_next2 = ri[s + 2 < K ? s + 2 : K - 1];
        if (ok) {
            if (!(pi_finite && fpfh_finite3(pjx, pjy, pjz))) {
                nonfinite = true;
            } else {
                const double dx = (double)pjx - (double)pix, dy = (double)pjy - (double)piy, dz = (double)pjz - (double)piz;
                const double d2 = fpfh_dot(dx, dy, dz, dx, dy, dz);
                const int mj = (int)((cur.w[SPFH_WORDS - 1] >> 8) & 0xFFu);
                if (d2 > 0.0 && d2 <= max_d2 && mj > 0) {
                    const double dm = (double)mj;
                    W += 1.0 / d2;
#pragma unroll
                    for (int k = 0; k < 33; ++k) {
                        const double c = (double)((cur.w[k >> 2] >> ((k & 3) * 8)) & 0xFFu);
                        A[k] += ((100.0 * c) / dm) / d2;
                    }
                }
            }
        }
        j = j_next; ok = ok_next; j_next = j_next2;
        pjx = pkx; pjy = pky; pjz = pkz;
        cur = nxt;
    }
    const int mi = (int)((own.w[SPFH_WORDS - 1] >> 8) & 0xFFu);
    const double dmi = (double)mi;
    float *o = out + row * 33;
#pragma unroll
    for (int k = 0; k < 33; ++k) {
        const double c = (double)((own.w[k >> 2] >> ((k & 3) * 8)) & 0xFFu);
        const double si = mi > 0 ? (100.0 * c) / dmi : 0.0;
        o[k] = (float)(si + (W > 0.0 ? A[k] / W : 0.0));
    }
    const int flags = (mi == 0 ? PN2_FPFH_ERR_EMPTY : 0) | (nonfinite ? PN2_FPFH_ERR_NONFINITE : 0);
    if (flags != 0 && err != nullptr) atomicOr(err, flags);
}

int fpfh_check(const void *points, int ldp, const void *idx, const void *io, int B, int M, int K, float max_d2) {
    PN2_CHECK_ARG(points && idx && io && B > 0 && M > 0 && B <= 65535 && M <= 0x7FFFFF00 && K >= 1);
    PN2_CHECK_ARG(ldp >= 3 && ldp <= 16 && max_d2 >= 0.f);       // (a NaN max_d2 fails the compare)
    PN2_CHECK_ARG(pn2_aligned(points, 4) && pn2_aligned(idx, 8));
    return K > 32 ? PN2_EUNSUPPORTED : PN2_OK;
}

}  // namespace

extern "C" {

int pn2_spfh(const float *points, int ldp, const float *normals, int ldn, int normal_col, const int64_t *idx, int B, int M, int K,
             float max_d2, const int64_t *n_points, uint8_t *spfh_out, int32_t *err, pn2_stream_t stream) {
    PN2_CHECK_ARG(normals && ldn >= 3 && ldn <= 16 && normal_col >= 0 && normal_col + 3 <= ldn);
    PN2_CHECK_ARG(pn2_aligned(normals, 4) && pn2_aligned(spfh_out, 4));
    const int rc = fpfh_check(points, ldp, idx, spfh_out, B, M, K, max_d2);
    if (rc != PN2_OK) return rc;
    const dim3 grid((unsigned)pn2_cdiv(M, FPFH_THREADS), B);
    hipLaunchKernelGGL(spfh_kernel, grid, dim3(FPFH_THREADS), 0, pn2_s(stream), points, ldp, normals + normal_col, ldn, idx, M, K,
                       (double)max_d2, n_points, reinterpret_cast<uint32_t *>(spfh_out), err);
    return pn2_launch_status();
}

int pn2_fpfh(const float *points, int ldp, const int64_t *idx, const uint8_t *spfh, int B, int M, int K, float max_d2,
             const int64_t *n_points, float *fpfh_out, int32_t *err, pn2_stream_t stream) {
    PN2_CHECK_ARG(spfh && pn2_aligned(spfh, 4) && pn2_aligned(fpfh_out, 4));
    const int rc = fpfh_check(points, ldp, idx, fpfh_out, B, M, K, max_d2);
    if (rc != PN2_OK) return rc;
    const dim3 grid((unsigned)pn2_cdiv(M, FPFH_THREADS), B);
    hipLaunchKernelGGL(fpfh_kernel, grid, dim3(FPFH_THREADS), 0, pn2_s(stream), points, ldp, idx, reinterpret_cast<const uint32_t *>(spfh),
                       M, K, (double)max_d2, n_points, fpfh_out, err);
    return pn2_launch_status();
}

}  // extern "C"
