// The criteria either side of the hot path.
// Negative log-likelihood over log-probabilities (reference semseg.py:143 `F.nll_loss(pred, target)`; partseg.py and the
// PointNet v1 losses call it the same way):
//     loss = - sum_r w[t_r] * logp[r, t_r] / sum_r w[t_r]      over rows with t_r != ignore_index
// ATen's own kernel for this reduction is a single workgroup (66 us forward + 37 us backward at 65 536 rows
// on MI355X, fully exposed between the forward and the backward pass); here every CU takes a slice, the
// per-workgroup partials are fp64 and the last workgroup to finish (ticket) adds them in a fixed order, so
// the result does not depend on the order the workgroups ran in.
// Cross entropy over logits (reference pcdseg.py:178-179, `nn.CrossEntropyLoss()(logits.transpose(2, 1), target)`: no weight,
// the input is the model's [B, N, C] output seen class-dim-1): log-softmax, NLL and label smoothing in one pass each way,
// with the same fp64 partials and ticket.
#include "pn2_common.h"
#include "softmax_row.h"

namespace {

constexpr int kThreads = 256;

// The tail of both criteria: every workgroup leaves its (numerator, denominator) as fp64 partials in ws [2][gridDim.x], the
// last one to arrive (ticket) adds them in a fixed order and writes *loss = num / den (mean) or num (!mean) and *denom = den.
// nan_without_den: a mean over den == 0 is NaN whatever num is (torch's cross entropy divides its NLL part, 0 then, and its
// smoothing part, which need not be 0, by the weight sum separately: NaN + inf).  Every thread of the workgroup must call it.
__device__ __forceinline__ void reduce_num_den(double num, double den, double *__restrict__ ws, unsigned *__restrict__ ticket,
                                               float *__restrict__ loss, float *__restrict__ denom, bool mean, bool nan_without_den) {
    __shared__ double sh[2][kThreads / 64];
    __shared__ bool last;
    num = pn2_wave_sum_f64(num);
    den = pn2_wave_sum_f64(den);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { sh[0][wave] = num; sh[1][wave] = den; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double n = 0.0, d = 0.0;
        for (int i = 0; i < kThreads / 64; ++i) { n += sh[0][i]; d += sh[1][i]; }
        ws[blockIdx.x] = n;
        ws[gridDim.x + blockIdx.x] = d;
        __threadfence();                                   // partials visible device-wide before the ticket
        last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    // <= 1024 partials: thread t adds partials t, t + 256, ... in index order, then a fixed-shape tree over the 256
    // threads -- the summation order is a function of gridDim only, never of which workgroup finished when.
    __shared__ double tree[2][kThreads];
    double n = 0.0, d = 0.0;
    for (unsigned i = threadIdx.x; i < gridDim.x; i += kThreads) {
        n += __builtin_nontemporal_load(ws + i);
        d += __builtin_nontemporal_load(ws + gridDim.x + i);
    }
    tree[0][threadIdx.x] = n;
    tree[1][threadIdx.x] = d;
    __syncthreads();
    for (int w = kThreads / 2; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) {
            tree[0][threadIdx.x] += tree[0][threadIdx.x + w];
            tree[1][threadIdx.x] += tree[1][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double n0 = tree[0][0];
        if (nan_without_den && tree[1][0] == 0.0) n0 = 0.0;
        *loss = (float)(mean ? n0 / tree[1][0] : tree[0][0]);                  // 0/0 = NaN when every row is ignored, as ATen
        *denom = (float)tree[1][0];
        *ticket = 0;                                       // the workspace is reusable without another memset
    }
}

__global__ __launch_bounds__(kThreads) void nll_fwd_kernel(const float *__restrict__ logp, int ld,
                                                           const int64_t *__restrict__ target,
                                                           const float *__restrict__ weight, int64_t R, int C,
                                                           int64_t ignore_index, double *__restrict__ ws,
                                                           unsigned *__restrict__ ticket, float *__restrict__ loss,
                                                           float *__restrict__ denom) {
    double num = 0.0, den = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < R; r += (int64_t)gridDim.x * kThreads) {
        const int64_t t = target[r];
        if (t == ignore_index) continue;
        if (t < 0 || t >= C) { num = __builtin_nan(""); continue; }      // ATen asserts; here the loss turns NaN
        const float w = weight ? weight[t] : 1.f;
        num -= (double)(w * logp[r * ld + t]);
        den += (double)w;
    }
    reduce_num_den(num, den, ws, ticket, loss, denom, true, false);
}

__global__ __launch_bounds__(kThreads) void nll_bwd_kernel(const int64_t *__restrict__ target,
                                                           const float *__restrict__ weight, int64_t R, int C,
                                                           int64_t ignore_index, const float *__restrict__ grad_loss,
                                                           const float *__restrict__ denom, float *__restrict__ dlogp,
                                                           int ld) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= R * ld) return;
    const int64_t r = i / ld;
    const int c = (int)(i - r * ld);
    const int64_t t = target[r];
    float v = 0.f;
    if (t == c && t < C && t != ignore_index) v = -(*grad_loss) * (weight ? weight[t] : 1.f) / *denom;
    dlogp[i] = v;
}

// log_softmax over the C leading columns of rows of pitch ldx (model/pointnet2.py:175, F.log_softmax(x, dim = -1) on the head's
// [B*N, classes] logits): one thread per row, the row read as float4 quads (a 13-class row of pitch 16 is one 64-byte line).
// ATen needs a copy (the logits arrive as a column slice of the padded GEMM output) plus its softmax kernel, and in the
// backward a zero fill plus a strided copy to re-pad the gradient; here both directions read and write the padded layout.
constexpr int kMaxClasses = 64;

__global__ __launch_bounds__(kThreads) void log_softmax_fwd_kernel(const float *__restrict__ x, int ldx, int64_t R, int C,
                                                                   float *__restrict__ out, int ldo) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= R) return;
    const float *row = x + r * ldx;
    float v[kMaxClasses];
    float m = -INFINITY;
#pragma unroll
    for (int q = 0; q < kMaxClasses / 4; ++q) {
        if (4 * q >= C) break;
        const float4 t = *reinterpret_cast<const float4 *>(row + 4 * q);     // ldx >= round4(C): the quad is inside the row
        v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
#pragma unroll
    for (int c = 0; c < kMaxClasses; ++c)
        if (c < C) m = fmaxf(m, v[c]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < kMaxClasses; ++c)
        if (c < C) s += expf(v[c] - m);
    const float lse = m + logf(s);
    float *o = out + r * ldo;
#pragma unroll
    for (int c = 0; c < kMaxClasses; ++c)
        if (c < C) o[c] = v[c] - lse;
}

// gx = g - exp(out) * sum(g) on the C leading columns of a row of pitch ldgx; the pad columns are written as zeros (the GEMM
// backward that consumes gx reads whole float4 quads)
__global__ __launch_bounds__(kThreads) void log_softmax_bwd_kernel(const float *__restrict__ g, int ldg, const float *__restrict__ out,
                                                                   int ldo, int64_t R, int C, float *__restrict__ gx, int ldgx) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= R) return;
    const float *gr = g + r * ldg, *orow = out + r * ldo;
    float gv[kMaxClasses];
    // the row sum as four interleaved partial sums: one running sum over 50..64 like-signed terms (the gradient of y.sum(), of a
    // per-row weight) carried 3..6 x the rounding error of ATen's tree-shaped sum into every gx through exp(out) * s
    float s4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < kMaxClasses; ++c)
        if (c < C) { gv[c] = gr[c]; s4[c & 3] += gv[c]; }
    const float s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    float *d = gx + r * ldgx;
#pragma unroll
    for (int c = 0; c < kMaxClasses; ++c) {
        if (c < C) d[c] = gv[c] - expf(orow[c]) * s;
        else if (c < ldgx) d[c] = 0.f;
    }
}


// ---------------------------------------------------------------------------------------------------------- cross entropy
// F.cross_entropy(input, target, weight, ignore_index, reduction, label_smoothing) with class-index targets (pcdseg.py:178-179).
// One thread per row r of C <= 64 logits, the row held in registers.  Two layouts, both read in place:
//   row-major      x[r * ld + c]                          (kRowQuads: ld % 4 == 0 and x 16-byte aligned, the row as float4 quads;
//                                                          kRowDwords: any pitch >= C)
//   class-strided  x[(r / inner) * C * inner + c * inner + r % inner]      [B, C, inner]: neighbouring lanes read neighbouring n
// With m = max_c x_c, d_c = x_c - m, s = sum_c exp(d_c):
//   l_r = (1 - eps) * w[t] * (log s - d_t) + eps / C * sum_c w[c] * (log s - d_c)
// The loss term is formed from d_t and log s, never as (m + log s) - x_t, which rounds at the magnitude of the logits (4.9e-4 on
// rows shifted by 1e4: the measured note in tests/test_loss_tail_gpu.py); for the same reason what the forward keeps for the
// backward is logsum[r] = log s, not m + log s: the backward re-takes the row maximum (exact, and the row is in registers
// anyway) and forms p_c = exp(d_c - log s).
enum { kRowQuads = 0, kRowDwords = 1, kClassStrided = 2 };
enum { kReduceNone = 0, kReduceMean = 1, kReduceSum = 2 };

template <int KC, int MODE>
__device__ __forceinline__ int64_t ce_row_base(int64_t r, int ld, int64_t inner, int C) {
    return MODE != kClassStrided ? r * ld : pn2_class_strided_base(r, inner, C);
}

template <int KC, int MODE>
__device__ __forceinline__ void ce_load_row(const float *__restrict__ row, int64_t inner, int C, float (&v)[KC]) {
    if (MODE == kRowQuads) {
#pragma unroll
        for (int q = 0; q < KC / 4; ++q) {
            if (4 * q + 3 < C) {
                const float4 t = *reinterpret_cast<const float4 *>(row + 4 * q);
                v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
            } else {                                                            // the last, partial quad: nothing past column C is read
#pragma unroll
                for (int c = 4 * q; c < 4 * q + 4; ++c)
                    if (c < C) v[c] = row[c];
            }
        }
    } else {
        pn2_load_row_strided<KC>(row, MODE == kClassStrided ? inner : 1, C, v);
    }
}

// the class weights (1 without a weight vector) in LDS, and their sum in a fixed order
__device__ __forceinline__ double ce_stage_weights(const float *__restrict__ weight, int C, float *wsh) {
    if ((int)threadIdx.x < kMaxClasses) wsh[threadIdx.x] = (int)threadIdx.x < C ? (weight ? weight[threadIdx.x] : 1.f) : 0.f;
    __syncthreads();
    double W = 0.0;
    for (int c = 0; c < C; ++c) W += (double)wsh[c];
    return W;
}

template <int KC, int MODE>
__global__ __launch_bounds__(kThreads) void ce_fwd_kernel(const float *__restrict__ x, int ld, int64_t inner,
                                                          const int64_t *__restrict__ target, const float *__restrict__ weight,
                                                          int64_t R, int C, int64_t ignore_index, double eps, int reduction,
                                                          double *__restrict__ ws, unsigned *__restrict__ ticket,
                                                          float *__restrict__ logsum, float *__restrict__ loss,
                                                          float *__restrict__ denom) {
    __shared__ float wsh[kMaxClasses];
    const double W = ce_stage_weights(weight, C, wsh);
    double num = 0.0, den = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < R; r += (int64_t)gridDim.x * kThreads) {
        asm volatile("" ::: "memory");      // keeps the weights in LDS: hoisted out of this loop they cost up to 64 more registers
        float v[KC];
        ce_load_row<KC, MODE>(x + ce_row_base<KC, MODE>(r, ld, inner, C), inner, C, v);
        const float logs = pn2_center_logsum<KC>(C, v);
        logsum[r] = logs;
        const int64_t t = target[r];
        double l = 0.0;
        if (t == ignore_index) {
        } else if (t < 0 || t >= C) {                              // never indexes the weights or the row
            l = __builtin_nan("");
            num = l;
        } else {
            float dt = 0.f;
#pragma unroll
            for (int c = 0; c < KC; ++c) dt = c == (int)t ? v[c] : dt;
            const double wt = (double)wsh[t];
            l = (1.0 - eps) * wt * ((double)logs - (double)dt);
            if (eps > 0.0) {
                float sw4[4] = {0.f, 0.f, 0.f, 0.f};                // sum_c w[c] * d_c, four interleaved partial sums
#pragma unroll
                for (int c = 0; c < KC; ++c)
                    if (c < C) sw4[c & 3] = fmaf(wsh[c], v[c], sw4[c & 3]);
                l += eps / (double)C * (W * (double)logs - ((double)(sw4[0] + sw4[1]) + (double)(sw4[2] + sw4[3])));
            }
            num += l;
            den += wt;
        }
        if (reduction == kReduceNone) loss[r] = (float)l;
    }
    if (reduction != kReduceNone) reduce_num_den(num, den, ws, ticket, loss, denom, reduction == kReduceMean, true);
}

// dx[r, c] = g_r * [(1 - eps) * w[t] * (p_c - [c == t]) + eps / C * (p_c * sum_k w[k] - w[c])], p_c = exp(d_c - logsum[r]);
// rows that are ignored or whose target is out of range are written as zeros; only the C logical columns of a row are written.
template <int KC, int MODE>
__global__ __launch_bounds__(kThreads) void ce_bwd_kernel(const float *__restrict__ x, int ld, int64_t inner,
                                                          const int64_t *__restrict__ target, const float *__restrict__ weight,
                                                          const float *__restrict__ logsum, int64_t R, int C,
                                                          int64_t ignore_index, float eps, int reduction,
                                                          const float *__restrict__ grad_out, const float *__restrict__ denom,
                                                          float *__restrict__ dx) {
    __shared__ float wsh[kMaxClasses];
    const float W = (float)ce_stage_weights(weight, C, wsh);
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= R) return;
    const int64_t base = ce_row_base<KC, MODE>(r, ld, inner, C);
    const int64_t t = target[r];
    float v[KC];
    if (t == ignore_index || t < 0 || t >= C) {
#pragma unroll
        for (int c = 0; c < KC; ++c) v[c] = 0.f;
    } else {
        ce_load_row<KC, MODE>(x + base, inner, C, v);
        float m = -INFINITY;
#pragma unroll
        for (int c = 0; c < KC; ++c)
            if (c < C) m = fmaxf(m, v[c]);
        const float logs = logsum[r];
        float g = reduction == kReduceNone ? grad_out[r] : *grad_out;
        if (reduction == kReduceMean) g /= *denom;
        const float a = g * (1.f - eps) * wsh[t], b = g * (eps / (float)C);
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            if (c >= C) continue;
            const float p = expf((v[c] - m) - logs);
            float d = a * (p - (c == (int)t ? 1.f : 0.f));
            if (eps > 0.f) d += b * (p * W - wsh[c]);
            v[c] = d;
        }
    }
    float *o = dx + base;
    if (MODE == kRowQuads) {
#pragma unroll
        for (int q = 0; q < KC / 4; ++q) {
            if (4 * q + 3 < C) {
                *reinterpret_cast<float4 *>(o + 4 * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
            } else {
#pragma unroll
                for (int c = 4 * q; c < 4 * q + 4; ++c)
                    if (c < C) o[c] = v[c];
            }
        }
    } else {
        const int64_t step = MODE == kClassStrided ? inner : 1;
#pragma unroll
        for (int c = 0; c < KC; ++c)
            if (c < C) o[c * step] = v[c];
    }
}

constexpr int kMaxBlocks = 1024;                           // workgroups of a reduced forward: the partials the last one adds

struct CeArgs {
    const float *x;
    int ld;
    int64_t inner;
    const int64_t *target;
    const float *weight;
    int64_t R;
    int C;
    int64_t ignore_index;
    double eps;
    int reduction;
};

// the argument rules the two launchers share; PN2_OK or PN2_EINVAL
int ce_check(const CeArgs &a) {
    PN2_CHECK_ARG(a.x && a.target && a.R > 0 && a.C > 0 && a.C <= kMaxClasses);
    PN2_CHECK_ARG(a.eps >= 0.0 && a.eps <= 1.0 && a.reduction >= kReduceNone && a.reduction <= kReduceSum);
    if (a.inner == 0) PN2_CHECK_ARG(a.ld >= a.C);
    else PN2_CHECK_ARG(a.inner > 0 && a.R % a.inner == 0);
    return PN2_OK;
}

int ce_mode(const void *p0, const void *p1, int ld, int64_t inner) {
    if (inner != 0) return kClassStrided;
    const bool aligned = (reinterpret_cast<uintptr_t>(p0) | reinterpret_cast<uintptr_t>(p1)) % 16 == 0;
    return ld % 4 == 0 && aligned ? kRowQuads : kRowDwords;
}

template <int KC, int MODE>
void ce_launch_fwd(const CeArgs &a, unsigned blocks, double *ws, unsigned *ticket, float *logsum, float *loss, float *denom,
                   hipStream_t s) {
    hipLaunchKernelGGL((ce_fwd_kernel<KC, MODE>), dim3(blocks), dim3(kThreads), 0, s, a.x, a.ld, a.inner, a.target, a.weight, a.R, a.C,
                       a.ignore_index, a.eps, a.reduction, ws, ticket, logsum, loss, denom);
}

template <int KC, int MODE>
void ce_launch_bwd(const CeArgs &a, const float *logsum, const float *grad_out, const float *denom, float *dx, hipStream_t s) {
    hipLaunchKernelGGL((ce_bwd_kernel<KC, MODE>), dim3((unsigned)pn2_cdiv(a.R, kThreads)), dim3(kThreads), 0, s, a.x, a.ld, a.inner,
                       a.target, a.weight, logsum, a.R, a.C, a.ignore_index, (float)a.eps, a.reduction, grad_out, denom, dx);
}

// rows of up to 16, 32 or 64 registers x the three addressing modes
#define PN2_CE_DISPATCH(C, mode, call, ...)                                                                      \
    do {                                                                                                          \
        if ((C) <= 16) {                                                                                          \
            if ((mode) == kRowQuads) call<16, kRowQuads>(__VA_ARGS__);                                            \
            else if ((mode) == kRowDwords) call<16, kRowDwords>(__VA_ARGS__);                                     \
            else call<16, kClassStrided>(__VA_ARGS__);                                                            \
        } else if ((C) <= 32) {                                                                                   \
            if ((mode) == kRowQuads) call<32, kRowQuads>(__VA_ARGS__);                                            \
            else if ((mode) == kRowDwords) call<32, kRowDwords>(__VA_ARGS__);                                     \
            else call<32, kClassStrided>(__VA_ARGS__);                                                            \
        } else {                                                                                                  \
            if ((mode) == kRowQuads) call<64, kRowQuads>(__VA_ARGS__);                                            \
            else if ((mode) == kRowDwords) call<64, kRowDwords>(__VA_ARGS__);                                     \
            else call<64, kClassStrided>(__VA_ARGS__);                                                            \
        }                                                                                                         \
    } while (0)

// The workspace of a reduced forward (NLL and cross-entropy alike): the workgroups' fp64 partials, numerators then denominators
// (gridDim.x <= kMaxBlocks of each), and the ticket word.
struct LossWork {
    double *partial;
    unsigned *ticket;
    int64_t bytes;
};
LossWork loss_work(void *base) {
    Pn2Arena a(base);
    return {a.take<double>(2 * kMaxBlocks), a.take<unsigned>(1), a.bytes()};
}

}  // namespace

extern "C" {

int pn2_log_softmax_fwd(const float *x, int ldx, int64_t R, int C, float *out, int ldo, pn2_stream_t stream) {
    PN2_CHECK_ARG(x && out && R > 0 && C > 0 && C <= kMaxClasses && ldx % 4 == 0 && ldx >= ((C + 3) & ~3) && ldo >= C);
    hipLaunchKernelGGL(log_softmax_fwd_kernel, dim3((unsigned)pn2_cdiv(R, kThreads)), dim3(kThreads), 0, pn2_s(stream), x, ldx, R, C, out, ldo);
    return pn2_launch_status();
}

int pn2_log_softmax_bwd(const float *grad_out, int ldg, const float *out, int ldo, int64_t R, int C, float *grad_x, int ldgx,
                        pn2_stream_t stream) {
    PN2_CHECK_ARG(grad_out && out && grad_x && R > 0 && C > 0 && C <= kMaxClasses && ldg >= C && ldo >= C && ldgx >= C && ldgx <= kMaxClasses);
    hipLaunchKernelGGL(log_softmax_bwd_kernel, dim3((unsigned)pn2_cdiv(R, kThreads)), dim3(kThreads), 0, pn2_s(stream), grad_out, ldg, out, ldo,
                       R, C, grad_x, ldgx);
    return pn2_launch_status();
}

int64_t pn2_nll_loss_workspace_bytes(int64_t R) {
    (void)R;
    return loss_work(nullptr).bytes;
}

int pn2_nll_loss_fwd(const float *logp, int ld, const int64_t *target, const float *weight, int64_t R, int C,
                     int64_t ignore_index, void *workspace, float *loss, float *denom, pn2_stream_t stream) {
    PN2_CHECK_ARG(logp && target && workspace && loss && denom && R > 0 && C > 0 && ld >= C);
    int64_t blocks = pn2_cdiv(R, kThreads);
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    const LossWork w = loss_work(workspace);
    hipLaunchKernelGGL(nll_fwd_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, pn2_s(stream), logp, ld, target, weight, R, C,
                       ignore_index, w.partial, w.ticket, loss, denom);
    return pn2_launch_status();
}

int pn2_nll_loss_bwd(const int64_t *target, const float *weight, int64_t R, int C, int64_t ignore_index,
                     const float *grad_loss, const float *denom, float *dlogp, int ld, pn2_stream_t stream) {
    PN2_CHECK_ARG(target && grad_loss && denom && dlogp && R > 0 && C > 0 && ld >= C);
    PN2_CHECK_ARG(R * ld < (1LL << 40));
    hipLaunchKernelGGL(nll_bwd_kernel, dim3((unsigned)pn2_cdiv(R * ld, kThreads)), dim3(kThreads), 0, pn2_s(stream), target,
                       weight, R, C, ignore_index, grad_loss, denom, dlogp, ld);
    return pn2_launch_status();
}

int64_t pn2_cross_entropy_workspace_bytes(int64_t R) {
    if (R <= 0) return PN2_EINVAL;
    return loss_work(nullptr).bytes;
}

int pn2_cross_entropy_fwd(const float *x, int ld, int64_t inner, const int64_t *target, const float *weight, int64_t R, int C,
                          int64_t ignore_index, double label_smoothing, int reduction, void *workspace, float *logsum, float *loss,
                          float *denom, pn2_stream_t stream) {
    const CeArgs a = {x, ld, inner, target, weight, R, C, ignore_index, label_smoothing, reduction};
    PN2_CHECK_ARG(ce_check(a) == PN2_OK && logsum && loss && (reduction == kReduceNone || (workspace && denom)));
    int64_t blocks = pn2_cdiv(R, kThreads);
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    const LossWork w = loss_work(workspace);                             // (null parts without a workspace: kReduceNone reads neither)
    const int mode = ce_mode(x, nullptr, ld, inner);
    PN2_CE_DISPATCH(C, mode, ce_launch_fwd, a, (unsigned)blocks, w.partial, w.ticket, logsum, loss, denom, pn2_s(stream));
    return pn2_launch_status();
}

int pn2_cross_entropy_bwd(const float *x, int ld, int64_t inner, const int64_t *target, const float *weight, const float *logsum,
                          int64_t R, int C, int64_t ignore_index, double label_smoothing, int reduction, const float *grad_out,
                          const float *denom, float *dx, pn2_stream_t stream) {
    const CeArgs a = {x, ld, inner, target, weight, R, C, ignore_index, label_smoothing, reduction};
    PN2_CHECK_ARG(ce_check(a) == PN2_OK && logsum && grad_out && dx && (reduction != kReduceMean || denom));
    PN2_CHECK_ARG(pn2_cdiv(R, kThreads) < (1LL << 31));
    const int mode = ce_mode(x, dx, ld, inner);
    PN2_CE_DISPATCH(C, mode, ce_launch_bwd, a, logsum, grad_out, denom, dx, pn2_s(stream));
    return pn2_launch_status();
}

}  // extern "C"
