// The image -> points direction of camera / LiDAR fusion: the colour of the pixel under each projected point, which is the first
// step of the reference's colour-generation task (data_utils/ColorGenerator_Loader.py:59-69), and the way back for looking at a
// prediction (the step the reference has commented out at :66-67).
//
//   pn2_sample_image   the per-point loop of ColorGenerator_Loader.py:63-65 (`pts_color[i] = frame_HSV[row, col]` for the points
//                      inside the frame) and the in-place float32 divisions of :68-69, for a batch of clouds that lie back to back
//                      in device memory, each reading its own image.  One thread per point: the pixel pair as one 8-byte load,
//                      the three image bytes as byte loads (the offset 3 (y W + x) has no alignment), three float stores into a
//                      row of any pitch.  Mode HSV converts the pixel by the integer rule stated in include/pn2.h (OpenCV's 8-bit
//                      BGR2HSV as remembered, UNVERIFIED against OpenCV); its two division tables are compile-time constants in
//                      constant memory.
//   pn2_hsv_to_rgb     normalised (h, s, v) rows -> uint8 pixels by this package's own fp64 rule (include/pn2.h).
//
// This file is built with -ffp-contract=off: every product, sum and division below is a separately rounded IEEE operation, and
// the float32 divisions are true divisions (numpy's `/=`), never reciprocal multiplies.
#include "pn2_common.h"

#include <limits.h>

namespace {

constexpr int kThreads = 256;

// rint(num / den) in fp64, round-half-even, for positive operands (the quotient is far below 2^31)
constexpr int rint_div(double num, double den) {
    const double q = num / den;
    const int lo = (int)q;
    const double frac = q - (double)lo;
    return frac > 0.5 ? lo + 1 : (frac < 0.5 ? lo : lo + (lo & 1));
}

struct HsvTables {
    int sdiv[256];                                  // rint(255 * 4096 / i), 0 at i = 0
    int hdiv[256];                                  // rint(180 * 4096 / (6 i)), 0 at i = 0
};
constexpr HsvTables make_tables() {
    HsvTables t = {};
    for (int i = 1; i < 256; ++i) {
        t.sdiv[i] = rint_div(255.0 * 4096.0, (double)i);
        t.hdiv[i] = rint_div(180.0 * 4096.0, 6.0 * (double)i);
    }
    return t;
}
__constant__ HsvTables c_hsv = make_tables();

template <bool HSV>
__global__ __launch_bounds__(kThreads) void sample_image_kernel(const int32_t *__restrict__ pix, const unsigned char *__restrict__ image,
                                                                int H, int W, int bgr, int normalize,
                                                                const int64_t *__restrict__ row_begin,
                                                                const int64_t *__restrict__ row_count, int64_t max_rows,
                                                                int64_t rows, float *__restrict__ out, int ldo,
                                                                unsigned char *__restrict__ valid, int *__restrict__ err) {
    const int b = blockIdx.y;
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    int64_t n = max_rows, begin = 0;
    if (row_count != nullptr) {
        const int64_t c = row_count[b];
        n = c < 0 ? 0 : (c > max_rows ? max_rows : c);
        begin = row_begin[b];
    }
    if (r >= n) return;
    if (begin < 0 || begin > rows - n) {                            // the cloud leaves the buffers: nothing of it is read or written
        if (r == 0 && err != nullptr) atomicOr(err, PN2_IMAGE_ERR_ROWS);
        return;
    }
    const int64_t row = begin + r;
    const int2 p = *reinterpret_cast<const int2 *>(pix + 2 * row);   // (x = column, y = row); INT32_MIN fails the test below
    const bool inside = p.y >= 0 && p.y < H && p.x >= 0 && p.x < W;
    float o0 = 0.f, o1 = 0.f, o2 = 0.f;
    if (inside) {
        const unsigned char *px = image + ((int64_t)b * H * W + ((int64_t)p.y * W + p.x)) * 3;
        const int c0 = px[0], c1 = px[1], c2 = px[2];
        const int cr = bgr ? c2 : c0, cg = c1, cb = bgr ? c0 : c2;
        if (!HSV) {
            o0 = (float)cr; o1 = (float)cg; o2 = (float)cb;
            if (normalize) { o0 = o0 / 255.0f; o1 = o1 / 255.0f; o2 = o2 / 255.0f; }
        } else {
            const int v = max(cr, max(cg, cb)), mn = min(cr, min(cg, cb));
            const int d = v - mn;
            const int s = (d * c_hsv.sdiv[v] + 2048) >> 12;
            const int h0 = (v == cr) ? cg - cb : (v == cg) ? cb - cr + 2 * d : cr - cg + 4 * d;
            int h = (h0 * c_hsv.hdiv[d] + 2048) >> 12;               // (an arithmetic shift: h0 may be negative)
            if (h < 0) h += 180;
            o0 = (float)h; o1 = (float)s; o2 = (float)v;
            if (normalize) { o0 = o0 / 180.0f; o1 = o1 / 255.0f; o2 = o2 / 255.0f; }
        }
    }
    float *dst = out + row * ldo;
    dst[0] = o0; dst[1] = o1; dst[2] = o2;
    if (valid != nullptr) valid[row] = inside ? 1 : 0;
}

// fp64 on the float32 inputs, every operation rounded separately, in the order include/pn2.h states.
__global__ __launch_bounds__(kThreads) void hsv_to_rgb_kernel(const float *__restrict__ hsv, int ld, int64_t N, int bgr,
                                                              unsigned char *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    const float *src = hsv + i * ld;
    const double h = (double)src[0];
    double s = (double)src[1], v = (double)src[2];
    unsigned char cr = 0, cg = 0, cb = 0;
    const double h6 = (h - floor(h)) * 6.0;                         // (an infinite h: inf - inf, NaN)
    if (h6 == h6 && s == s && v == v) {
        s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
        v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
        const int k = min((int)h6, 5);                              // (h - floor(h) may round up to 1.0: sector 5, f = 1)
        const double f = h6 - (double)k;
        const double p = v * (1.0 - s), q = v * (1.0 - s * f), t = v * (1.0 - s * (1.0 - f));
        double r, g, bl;
        switch (k) {
            case 0: r = v; g = t; bl = p; break;
            case 1: r = q; g = v; bl = p; break;
            case 2: r = p; g = v; bl = t; break;
            case 3: r = p; g = q; bl = v; break;
            case 4: r = t; g = p; bl = v; break;
            default: r = v; g = p; bl = q; break;
        }
        cr = (unsigned char)(int)rint(255.0 * r);                   // (round-half-even; the operands are in [0, 255])
        cg = (unsigned char)(int)rint(255.0 * g);
        cb = (unsigned char)(int)rint(255.0 * bl);
    }
    unsigned char *dst = out + 3 * i;
    dst[0] = bgr ? cb : cr; dst[1] = cg; dst[2] = bgr ? cr : cb;
}

}  // namespace

extern "C" {

int pn2_sample_image(const int32_t *pix, const uint8_t *image, int B, int H, int W, int channel_order, int mode, int normalize,
                     const int64_t *row_begin, const int64_t *row_count, int64_t max_rows, int64_t rows, float *out, int ldo,
                     uint8_t *valid, int *err, pn2_stream_t stream) {
    PN2_CHECK_ARG(pix && image && out && B >= 1 && B <= 65535 && H > 0 && W > 0 && ldo >= 3);
    PN2_CHECK_ARG((int64_t)H * W * 3 < (int64_t)1 << 31);
    PN2_CHECK_ARG((channel_order == PN2_CHANNELS_RGB || channel_order == PN2_CHANNELS_BGR) &&
                  (mode == PN2_IMAGE_RGB || mode == PN2_IMAGE_HSV) && (normalize == 0 || normalize == 1));
    PN2_CHECK_ARG(max_rows >= 0 && max_rows < (int64_t)1 << 31 && (row_begin == nullptr) == (row_count == nullptr));
    PN2_CHECK_ARG((row_count != nullptr || B == 1) && pn2_aligned(pix, 8) && rows >= max_rows);
    if (max_rows == 0) return PN2_OK;
    const dim3 grid((unsigned)pn2_cdiv(max_rows, kThreads), (unsigned)B);
    if (mode == PN2_IMAGE_HSV)
        hipLaunchKernelGGL(sample_image_kernel<true>, grid, dim3(kThreads), 0, pn2_s(stream), pix, image, H, W, channel_order,
                           normalize, row_begin, row_count, max_rows, rows, out, ldo, valid, err);
    else
        hipLaunchKernelGGL(sample_image_kernel<false>, grid, dim3(kThreads), 0, pn2_s(stream), pix, image, H, W, channel_order,
                           normalize, row_begin, row_count, max_rows, rows, out, ldo, valid, err);
    return pn2_launch_status();
}

int pn2_hsv_to_rgb(const float *hsv, int ld, int64_t N, int channel_order, uint8_t *out, pn2_stream_t stream) {
    PN2_CHECK_ARG(ld >= 3 && N >= 0 && (N == 0 || (hsv && out)));
    PN2_CHECK_ARG(channel_order == PN2_CHANNELS_RGB || channel_order == PN2_CHANNELS_BGR);
    if (N == 0) return PN2_OK;
    const int64_t blocks = pn2_cdiv(N, kThreads);
    PN2_CHECK_ARG(blocks <= 0x7fffffff);
    hipLaunchKernelGGL(hsv_to_rgb_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, pn2_s(stream), hsv, ld, N, channel_order, out);
    return pn2_launch_status();
}

}  // extern "C"
