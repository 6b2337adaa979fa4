// Segmentation metrics: the confusion table of a batch of log-probabilities against its labels, the one statistic behind the
// reference's evaluation loops (pcd_utils.py:79-113 compute_cat_iou / calc_categorical_iou, :65-77, :132-210 and
// pcdseg.py:58-97).  The reference takes an arg-max, then per class four elementwise passes over [B, N] and two blocking reads;
// here ONE pass over the rows produces, per cloud (or pooled over the batch), the integer table
//     conf[t, c] = number of rows with target t whose prediction is c,        t in [0, C);
//     conf[C, c] = the same for rows whose target is no class (t < 0 or t >= C),
// from which every intersection, union and accuracy follows on integers (pointnet12_amd/metrics.py).
//
// Prediction (the contract, include/pn2.h): the index of the row's largest entry among its first C columns, the LOWEST index on
// equal values; a NaN counts as largest and the first NaN wins; a row of all -inf predicts 0 -- what torch.max(dim)[1] and
// argmax return (row_argmax.h, shared with view.hip).  Columns c >= C of a padded row are read (float4 quads) but never compared.
//
// A thread owns a row.  Labels of neighbouring points are mostly equal, so the lanes of a wave mostly hit one bin: up to
// kAggregateRounds bins are counted per wave with a ballot and added by one lane, whatever is left goes one lane at a time.  The
// counts go into a per-wave copy of the table in LDS (32-bit; a workgroup never sees 2^32 rows), and only the non-zero bins are
// flushed with 64-bit integer atomics: integer adds commute, the table is bit-identical however the workgroups were scheduled.
#include "pn2_common.h"
#include "row_argmax.h"
#include "wave_ops.h"

#include <algorithm>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / PN2_WAVE;
constexpr int kMaxClasses = 64;
constexpr int kAggregateRounds = 4;
constexpr int kMaxStaticLds = 64 * 1024;

// Table copies in LDS: one per wave while four of them fit the 64 KiB a workgroup gets without asking (C <= 63), two at C = 64.
inline int table_copies(int C) { return 4 * (C + 1) * C * (int)sizeof(unsigned) <= kMaxStaticLds ? kWaves : 2; }

// grid: B * wgs_per_cloud workgroups; workgroup w of a cloud takes the rows n = w * 256 + thread + i * wgs_per_cloud * 256.
template <bool QUADS>
__global__ __launch_bounds__(kThreads) void seg_confusion_kernel(const float *__restrict__ logp, int ld, const int64_t *__restrict__ target,
                                                                 int64_t N, int C, int64_t ignore_index, int wgs_per_cloud, int copies,
                                                                 int64_t *__restrict__ conf, int64_t conf_stride,
                                                                 int64_t *__restrict__ pred) {
    extern __shared__ unsigned table[];                       // [copies][(C + 1) * C]
    const int bins = (C + 1) * C;
    for (int e = threadIdx.x; e < copies * bins; e += kThreads) table[e] = 0u;
    __syncthreads();

    const int b = blockIdx.x / wgs_per_cloud, w = blockIdx.x - b * wgs_per_cloud;
    const int lane = threadIdx.x & (PN2_WAVE - 1);
    unsigned *mine = table + ((threadIdx.x >> 6) % copies) * bins;
    const int64_t stride = (int64_t)wgs_per_cloud * kThreads;
    const int64_t trips = (N - (int64_t)w * kThreads + stride - 1) / stride;        // the same for every thread of the workgroup (>= 1)
    for (int64_t i = 0; i < trips; ++i) {
        const int64_t n = (int64_t)w * kThreads + i * stride + threadIdx.x;
        bool live = n < N;
        int bin = 0;
        if (live) {
            const int64_t r = (int64_t)b * N + n;
            const float *row = logp + r * ld;
            float best;
            const int arg = pn2_row_argmax<QUADS>(row, C, best);
            if (pred != nullptr) pred[r] = arg;
            const int64_t t = target[r];
            live = t != ignore_index;
            bin = (t >= 0 && t < C ? (int)t : C) * C + arg;
        }
        live = pn2_wave_combine<kAggregateRounds>(bin, live, [&](bool, int leader, unsigned long long votes) {
            if (lane == leader) atomicAdd(mine + bin, (unsigned)__popcll(votes));
        });
        if (live) atomicAdd(mine + bin, 1u);
    }
    __syncthreads();

    unsigned long long *dst = reinterpret_cast<unsigned long long *>(conf + (int64_t)b * conf_stride);
    for (int e = threadIdx.x; e < bins; e += kThreads) {
        unsigned long long sum = 0ull;
        for (int k = 0; k < copies; ++k) sum += table[k * bins + e];
        if (sum != 0ull) atomicAdd(dst + e, sum);
    }
}

}  // namespace

extern "C" {

int pn2_seg_confusion(const float *logp, int ld, const int64_t *target, int B, int64_t N, int C, int64_t ignore_index, int64_t *conf,
                      int64_t conf_stride, int64_t *pred, pn2_stream_t stream) {
    PN2_CHECK_ARG(logp && target && conf && ld > 0 && B >= 0 && N >= 0 && C > 0 && conf_stride >= 0);
    if (C > kMaxClasses) return PN2_EUNSUPPORTED;
    PN2_CHECK_ARG(ld >= C && (conf_stride == 0 || conf_stride >= (int64_t)(C + 1) * C));
    if (B == 0 || N == 0) return PN2_OK;
    PN2_CHECK_ARG(N < (int64_t)1 << 40 && (int64_t)B * N < (int64_t)1 << 48);
    // enough workgroups to fill the chip a few times over, each on rows of ONE cloud, none with 2^32 rows (32-bit LDS counters)
    const int64_t want = pn2_cdiv(8 * (int64_t)pn2_num_cus(), B);
    const int64_t wgs = std::max<int64_t>(std::min<int64_t>(pn2_cdiv(N, kThreads), want), pn2_cdiv(N, (int64_t)1 << 31));
    PN2_CHECK_ARG(wgs * B < (int64_t)1 << 31);
    const int copies = table_copies(C);
    const size_t lds = (size_t)copies * (C + 1) * C * sizeof(unsigned);
    const bool quads = ld % 4 == 0 && (reinterpret_cast<uintptr_t>(logp) & 15) == 0;
    hipStream_t s = pn2_s(stream);
    if (quads)
        hipLaunchKernelGGL(seg_confusion_kernel<true>, dim3((unsigned)(wgs * B)), dim3(kThreads), lds, s, logp, ld, target, N, C,
                           ignore_index, (int)wgs, copies, conf, conf_stride, pred);
    else
        hipLaunchKernelGGL(seg_confusion_kernel<false>, dim3((unsigned)(wgs * B)), dim3(kThreads), lds, s, logp, ld, target, N, C,
                           ignore_index, (int)wgs, copies, conf, conf_stride, pred);
    return pn2_launch_status();
}

}  // extern "C"
