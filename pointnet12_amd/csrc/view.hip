// The second half of the reference's KITTI demo frame (pcdvis.py:115-144) on the device: class prediction with optional class
// merging, projection of the points into the camera image, and drawing them as filled discs.
//
//   pn2_seg_predict      logits[0].argmax(-1) (pcdvis.py:136) and the class merges of KITTI_2_Common / SemKITTI_2_Common
//                        (data_utils/kitti_utils.py:41-58, :92-117): one thread per row, the arg-max of row_argmax.h (shared
//                        with metrics.hip) over the classes or over the groups' maxima.
//   pn2_project_points   Semantic_KITTI_Utils.project_3d_to_2d (kitti_utils.py:313-336) in numpy's own arithmetic, and the top
//                        view's pixel coordinates (:387-389) in Python's.  This file is built with -ffp-contract=off: every
//                        product and sum below is a separately rounded IEEE operation, as numpy's and Python's are.
//   pn2_splat_discs /    draw_2d_points / draw_2d_top_view (:368-392).  The reference draws the points one after another, so a
//   pn2_splat_resolve    pixel shows the LAST point that covered it: here that order is an integer maximum, owner[p] = max(i + 1)
//                        over the points i whose disc covers p (non-returning 32-bit atomics), and a second pass colours every
//                        pixel from its owner's label.  Integer maxima commute: the image is bit-identical from run to run.
//   pn2_depth_splat /    the 3-D ego view, Window_Manager.update (pcdvis.py:31-51, :143): the scan seen through a fixed pinhole
//   pn2_depth_resolve    camera, drawn as square points of integer size with a depth test.  Here the depth test is an integer
//                        minimum of (float32 depth bits, point index) per pixel (non-returning 64-bit atomics): the nearest
//                        point wins, the lowest index among equal depths (GL_LESS in draw order); minima commute as well.
//
// Small tables (calibration, merge groups, the disc's row half-widths) are HOST arrays: they are validated on the host and
// travel inside the launch's arguments, so no entry point allocates, copies or waits, and every call can be captured in a graph.
#include "pn2_common.h"
#include "row_argmax.h"

#include <limits.h>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxClasses = 64;
constexpr int kMaxGroups = 64;
constexpr int kMaxMembers = 256;
constexpr int kMaxStencilRows = 65;             // radius <= 32

struct GroupTable {
    int begin[kMaxGroups + 1];
    unsigned char member[kMaxMembers];
};
struct Calib {
    double RT[12];
    double P[9];
};
struct Stencil {
    int half_width[kMaxStencilRows];
};
struct Pinhole {
    double E[12];                               // [R | t], row-major
    double fx, fy, cx, cy;
    double z_near, z_far;
};
constexpr int kMaxPointSize = 16;
constexpr unsigned long long kEmptyKey = ~0ull;

// ------------------------------------------------------------------------------------------------------------------ predict
// Tensor.max(dim) of a group's members: the largest, NaN if any member is NaN (the first one met is returned).
template <bool QUADS>
__global__ __launch_bounds__(kThreads) void seg_predict_kernel(const float *__restrict__ logp, int ld, int64_t R, int C, int G,
                                                               GroupTable tab, int64_t *__restrict__ pred,
                                                               float *__restrict__ merged, int ldm) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= R) return;
    const float *row = logp + r * ld;
    if (G == 0) {
        float best;
        const int arg = pn2_row_argmax<QUADS>(row, C, best);
        if (pred != nullptr) pred[r] = arg;
        return;
    }
    float best = 0.f;
    int arg = 0;
    for (int g = 0; g < G; ++g) {                                   // (uniform: the table is read through scalar loads)
        float v = row[tab.member[tab.begin[g]]];
        for (int k = tab.begin[g] + 1; k < tab.begin[g + 1]; ++k) {
            const float m = row[tab.member[k]];
            if (pn2_beats(m, v)) v = m;
        }
        if (merged != nullptr) merged[r * ldm + g] = v;
        if (g == 0 || pn2_beats(v, best)) { best = v; arg = g; }
    }
    if (pred != nullptr) pred[r] = arg;
}

// ------------------------------------------------------------------------------------------------------------------ project
__device__ __forceinline__ bool fits_int32(float v) { return v == v && fabsf(v) < 2147483648.f; }     // finite and |v| < 2^31

// np.matmul(RT, [x, y, z, 1]) and np.matmul(P, c) of kitti_utils.py:322-329: fp64 products added left to right, each result
// stored into the float32 array it came from; then the fp32 division of :332.
__global__ __launch_bounds__(kThreads) void project_kernel(const float *__restrict__ xyz, int ldx, int64_t N, Calib cal,
                                                           float *__restrict__ pts_2d, int32_t *__restrict__ pix) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    const float *p = xyz + i * ldx;
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    float c[3], q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        c[k] = (float)(((cal.RT[4 * k] * x + cal.RT[4 * k + 1] * y) + cal.RT[4 * k + 2] * z) + cal.RT[4 * k + 3] * 1.0);
#pragma unroll
    for (int k = 0; k < 3; ++k)
        q[k] = (float)((cal.P[3 * k] * (double)c[0] + cal.P[3 * k + 1] * (double)c[1]) + cal.P[3 * k + 2] * (double)c[2]);
    const float u = q[0] / q[2], v = q[1] / q[2];
    if (pts_2d != nullptr) {
        pts_2d[2 * i] = u;
        pts_2d[2 * i + 1] = v;
    }
    if (pix != nullptr) {
        const bool ok = fits_int32(u) && fits_int32(v);
        pix[2 * i] = ok ? (int32_t)u : INT_MIN;                      // (a float -> int conversion truncates toward zero)
        pix[2 * i + 1] = ok ? (int32_t)v : INT_MIN;
    }
}

// X = int(-x*800 + 600), Y = int(-y*800 + 400) of kitti_utils.py:388-389 on Python floats (fp64); the centre is (Y, X) as :390
// passes it to cv2.circle.
__global__ __launch_bounds__(kThreads) void top_view_kernel(const float *__restrict__ xyz, int ldx, int64_t N,
                                                            int32_t *__restrict__ pix) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    const float *p = xyz + i * ldx;
    const double X = -(double)p[0] * 800.0 + 600.0, Y = -(double)p[1] * 800.0 + 400.0;
    const bool ok = X == X && Y == Y && fabs(X) < 2147483648.0 && fabs(Y) < 2147483648.0;
    pix[2 * i] = ok ? (int32_t)Y : INT_MIN;
    pix[2 * i + 1] = ok ? (int32_t)X : INT_MIN;
}

// -------------------------------------------------------------------------------------------------------------------- splat
// One thread per (point, stencil row): row dy of point i covers the pixels (cy + dy, cx - hw .. cx + hw), clipped to the image.
// Coordinates are widened to 64 bits before anything is added to them: a centre may sit anywhere in int32.
__global__ __launch_bounds__(kThreads) void splat_discs_kernel(const int32_t *__restrict__ pix, int64_t N, Stencil st, int rows,
                                                               int H, int W, unsigned *__restrict__ owner) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= N * rows) return;
    const int64_t i = t / rows;
    const int j = (int)(t - i * rows);
    const int32_t cx = pix[2 * i], cy = pix[2 * i + 1];
    if (cx == INT_MIN || cy == INT_MIN) return;
    const int hw = st.half_width[j];
    const int64_t y = (int64_t)cy + (j - rows / 2);
    if (hw < 0 || y < 0 || y >= H) return;
    const int64_t lo = (int64_t)cx - hw, hi = (int64_t)cx + hw;
    const int64_t x0 = lo < 0 ? 0 : lo, x1 = hi > W - 1 ? W - 1 : hi;
    unsigned *line = owner + y * W;
    const unsigned id = (unsigned)i + 1u;
    for (int64_t x = x0; x <= x1; ++x)
        (void)__hip_atomic_fetch_max(line + x, id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // result unused: non-returning
}

__global__ __launch_bounds__(kThreads) void splat_resolve_kernel(const unsigned *__restrict__ owner, int64_t pixels,
                                                                 const int64_t *__restrict__ label, int64_t N,
                                                                 const unsigned char *__restrict__ colors, int C,
                                                                 const unsigned char *__restrict__ background,
                                                                 unsigned char *__restrict__ out, int *__restrict__ err) {
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= pixels) return;
    unsigned char r = 0, g = 0, b = 0;
    if (background != nullptr) { r = background[3 * p]; g = background[3 * p + 1]; b = background[3 * p + 2]; }
    const unsigned o = owner[p];
    if (o != 0u && (int64_t)o <= N) {
        const int64_t l = label[o - 1u];
        if (l >= 0 && l < C) {
            r = colors[3 * l]; g = colors[3 * l + 1]; b = colors[3 * l + 2];
        } else if (err != nullptr) {
            atomicOr(err, 1);                                       // (the reference's colors[pred] raises IndexError)
        }
    }
    out[3 * p] = r; out[3 * p + 1] = g; out[3 * p + 2] = b;
}

// ---------------------------------------------------------------------------------------------------------------- depth test
// One thread per (point, row of its square).  fp64 on the widened fp32 coordinates, every product and sum rounded separately and in
// the order include/pn2.h states (this file is built with -ffp-contract=off).  The centre is compared as a double before anything
// is converted to an integer: below 2^30 in magnitude, floor() and the half size fit 64 bits with room to spare.
__global__ __launch_bounds__(kThreads) void depth_splat_kernel(const float *__restrict__ xyz, int ldx, int64_t N, Pinhole cam, int s,
                                                               int H, int W, unsigned long long *__restrict__ zkey) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= N * s) return;
    const int64_t i = t / s;
    const int j = (int)(t - i * s);
    const float *p = xyz + i * ldx;
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    double c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = ((cam.E[4 * k] * x + cam.E[4 * k + 1] * y) + cam.E[4 * k + 2] * z) + cam.E[4 * k + 3];
    const double Z = c[2];
    if (!(cam.z_near < Z && Z < cam.z_far)) return;                 // (a NaN depth fails both)
    const float d = (float)Z;                                       // finite and not negative: its bits order like its value
    const double xw = ((cam.fx * c[0]) / Z + cam.cx) + 0.5, yw = ((cam.fy * c[1]) / Z + cam.cy) + 0.5;
    if (!(fabs(xw) < 1073741824.0) || !(fabs(yw) < 1073741824.0)) return;      // not finite, or 2^30 and beyond
    const double half = (s & 1) ? 0.0 : 0.5;
    const int64_t row = (int64_t)floor(yw + half) - s / 2 + j;
    if (row < 0 || row >= H) return;
    const int64_t lo = (int64_t)floor(xw + half) - s / 2, hi = lo + s - 1;
    const int64_t x0 = lo < 0 ? 0 : lo, x1 = hi > W - 1 ? W - 1 : hi;
    unsigned long long *line = zkey + row * W;
    const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)i;
    for (int64_t col = x0; col <= x1; ++col)
        (void)__hip_atomic_fetch_min(line + col, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // result unused: non-returning
}

__global__ __launch_bounds__(kThreads) void depth_resolve_kernel(const unsigned long long *__restrict__ zkey, int64_t pixels,
                                                                 unsigned *__restrict__ owner, float *__restrict__ depth) {
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= pixels) return;
    const unsigned long long key = zkey[p];
    const bool empty = key == kEmptyKey;
    if (owner != nullptr) owner[p] = empty ? 0u : (unsigned)key + 1u;
    if (depth != nullptr) depth[p] = empty ? __uint_as_float(0x7f800000u) : __uint_as_float((unsigned)(key >> 32));
}

}  // namespace

extern "C" {

int pn2_seg_predict(const float *logp, int ld, int64_t R, int C, const int32_t *group_begin, const int32_t *member, int G,
                    int64_t *pred, float *merged, int ldm, pn2_stream_t stream) {
    PN2_CHECK_ARG(logp && ld > 0 && R >= 0 && C > 0 && G >= 0);
    if (C > kMaxClasses || G > kMaxGroups) return PN2_EUNSUPPORTED;
    PN2_CHECK_ARG(ld >= C && (G == 0 ? merged == nullptr : (group_begin && member)) && (merged == nullptr || ldm >= G));
    GroupTable tab = {};
    if (G > 0) {
        PN2_CHECK_ARG(group_begin[0] == 0);
        for (int g = 0; g < G; ++g) PN2_CHECK_ARG(group_begin[g + 1] > group_begin[g]);              // no empty group
        if (group_begin[G] > kMaxMembers) return PN2_EUNSUPPORTED;
        for (int g = 0; g <= G; ++g) tab.begin[g] = group_begin[g];
        for (int k = 0; k < group_begin[G]; ++k) {
            PN2_CHECK_ARG(member[k] >= 0 && member[k] < C);
            tab.member[k] = (unsigned char)member[k];
        }
    }
    if (R == 0 || (pred == nullptr && merged == nullptr)) return PN2_OK;
    const int64_t blocks = pn2_cdiv(R, kThreads);
    PN2_CHECK_ARG(blocks <= 0x7fffffff);
    const bool quads = G == 0 && ld % 4 == 0 && pn2_aligned(logp, 16);
    if (quads)
        hipLaunchKernelGGL(seg_predict_kernel<true>, dim3((unsigned)blocks), dim3(kThreads), 0, pn2_s(stream), logp, ld, R, C, G, tab,
                           pred, merged, ldm);
    else
        hipLaunchKernelGGL(seg_predict_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, pn2_s(stream), logp, ld, R, C, G, tab,
                           pred, merged, ldm);
    return pn2_launch_status();
}

int pn2_project_points(const float *xyz, int ldx, int64_t N, const double *RT, const double *P, float *pts_2d, int32_t *pix,
                       pn2_stream_t stream) {
    PN2_CHECK_ARG(xyz && ldx >= 3 && N >= 0 && (RT == nullptr) == (P == nullptr));
    PN2_CHECK_ARG(RT != nullptr ? (pts_2d != nullptr || pix != nullptr) : (pts_2d == nullptr && pix != nullptr));
    if (N == 0) return PN2_OK;
    const int64_t blocks = pn2_cdiv(N, kThreads);
    PN2_CHECK_ARG(blocks <= 0x7fffffff);
    if (RT == nullptr) {
        hipLaunchKernelGGL(top_view_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, pn2_s(stream), xyz, ldx, N, pix);
        return pn2_launch_status();
    }
    Calib cal;
    for (int k = 0; k < 12; ++k) cal.RT[k] = RT[k];
    for (int k = 0; k < 9; ++k) cal.P[k] = P[k];
    hipLaunchKernelGGL(project_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, pn2_s(stream), xyz, ldx, N, cal, pts_2d, pix);
    return pn2_launch_status();
}

int pn2_splat_discs(const int32_t *pix, int64_t N, const int32_t *half_width, int radius, int H, int W, uint32_t *owner,
                    pn2_stream_t stream) {
    PN2_CHECK_ARG(half_width && radius >= 0 && H > 0 && W > 0 && owner && N >= 0 && (N == 0 || pix));
    if (2 * radius + 1 > kMaxStencilRows) return PN2_EUNSUPPORTED;
    PN2_CHECK_ARG((int64_t)H * W < (int64_t)1 << 31 && N < (int64_t)1 << 31);
    const int rows = 2 * radius + 1;
    Stencil st = {};
    for (int j = 0; j < rows; ++j) {
        PN2_CHECK_ARG(half_width[j] >= -1 && half_width[j] <= 32767);                                // -1: an empty row
        st.half_width[j] = half_width[j];
    }
    pn2_fill_u32(owner, 0u, (int64_t)H * W, pn2_s(stream));         // (a kernel, not a memset node: see pn2_common.h)
    if (N > 0) {
        const int64_t blocks = pn2_cdiv(N * rows, kThreads);
        PN2_CHECK_ARG(blocks <= 0x7fffffff);
        hipLaunchKernelGGL(splat_discs_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, pn2_s(stream), pix, N, st, rows, H, W,
                           owner);
    }
    return pn2_launch_status();
}

int pn2_splat_resolve(const uint32_t *owner, int H, int W, const int64_t *label, int64_t N, const uint8_t *colors, int C,
                      const uint8_t *background, uint8_t *out, int *err, pn2_stream_t stream) {
    PN2_CHECK_ARG(owner && out && H > 0 && W > 0 && N >= 0 && C >= 0 && (N == 0 || (label && colors)));
    PN2_CHECK_ARG((int64_t)H * W < (int64_t)1 << 31 && N < (int64_t)1 << 31);
    const int64_t pixels = (int64_t)H * W;
    hipLaunchKernelGGL(splat_resolve_kernel, dim3((unsigned)pn2_cdiv(pixels, kThreads)), dim3(kThreads), 0, pn2_s(stream), owner,
                       pixels, label, N, colors, C, background, out, err);
    return pn2_launch_status();
}

int pn2_depth_splat(const float *xyz, int ldx, int64_t N, const double *extrinsic, const double *intrinsic, double z_near,
                    double z_far, int point_size, int H, int W, uint64_t *zkey, pn2_stream_t stream) {
    PN2_CHECK_ARG(ldx >= 3 && N >= 0 && (N == 0 || xyz) && extrinsic && intrinsic && H > 0 && W > 0 && zkey);
    PN2_CHECK_ARG((int64_t)H * W < (int64_t)1 << 31 && N < (int64_t)1 << 31);
    PN2_CHECK_ARG(0.0 < z_near && z_near < z_far && z_far <= 3e38);                                  // (NaN planes fail)
    if (point_size < 1 || point_size > kMaxPointSize) return PN2_EUNSUPPORTED;
    pn2_fill_u32(zkey, 0xffffffffu, 2 * (int64_t)H * W, pn2_s(stream));     // (a kernel, not a memset node: see pn2_common.h)
    if (N > 0) {
        Pinhole cam;
        for (int k = 0; k < 12; ++k) cam.E[k] = extrinsic[k];
        cam.fx = intrinsic[0]; cam.fy = intrinsic[1]; cam.cx = intrinsic[2]; cam.cy = intrinsic[3];
        cam.z_near = z_near; cam.z_far = z_far;
        const int64_t blocks = pn2_cdiv(N * point_size, kThreads);
        PN2_CHECK_ARG(blocks <= 0x7fffffff);
        hipLaunchKernelGGL(depth_splat_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, pn2_s(stream), xyz, ldx, N, cam, point_size,
                           H, W, reinterpret_cast<unsigned long long *>(zkey));
    }
    return pn2_launch_status();
}

int pn2_depth_resolve(const uint64_t *zkey, int H, int W, uint32_t *owner, float *depth, pn2_stream_t stream) {
    PN2_CHECK_ARG(zkey && H > 0 && W > 0 && (int64_t)H * W < (int64_t)1 << 31);
    if (owner == nullptr && depth == nullptr) return PN2_OK;
    const int64_t pixels = (int64_t)H * W;
    hipLaunchKernelGGL(depth_resolve_kernel, dim3((unsigned)pn2_cdiv(pixels, kThreads)), dim3(kThreads), 0, pn2_s(stream),
                       reinterpret_cast<const unsigned long long *>(zkey), pixels, owner, depth);
    return pn2_launch_status();
}

}  // extern "C"
