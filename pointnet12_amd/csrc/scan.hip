// Scan ingest on the device: Semantic_KITTI_Utils.get (data_utils/kitti_utils.py:183-227) with points_basic_filter (:259-280)
// for a batch of raw scans that lie back to back in HBM -- the class map, the drop of class 0, the field-of-view / range-box
// test and the boolean-index compaction, without a host pass and with the kept count left in device memory.
//
//   pn2_scan_filter   the stable tile compaction of compact.h (three plain launches on the caller's stream: flags, offsets, write):
//     scan_flag_kernel     keeps a row by the rule of include/pn2.h (class map, drop of class 0, view / box test);
//     scan_write_kernel    moves every kept row as one 16-byte load and one 16-byte store, with its class and its row number.
//   The output is points[mask], in scan order, byte-identical from run to run.
//
// This file is built with -ffp-contract=off: d = sqrt((x*x + y*y) + z*z) is three separately rounded fp32 operations and a
// correctly rounded square root, as numpy's np.sqrt(x**2 + y**2 + z**2) is.  The two angles are fp64 atan2 values rounded to
// float32 (a definite rule; numpy's float32 arctan2 is not correctly rounded and differs between builds).
#include "compact.h"

namespace {

struct Rule {
    float fov[4];                                                   // t0 < az < t1, t2 < el < t3
    float box[8];                                                   // x, y, z, d: lower, upper
    int has_fov, has_box;
};

__device__ __forceinline__ bool geometry_keeps(const float4 p, const Rule &rule) {
    const float x = p.x, y = p.y, z = p.z;
    const float d = __fsqrt_rn((x * x + y * y) + z * z);
    if (rule.has_box &&
        !(x > rule.box[0] && x < rule.box[1] && y > rule.box[2] && y < rule.box[3] && z > rule.box[4] && z < rule.box[5] &&
          d > rule.box[6] && d < rule.box[7]))
        return false;                                               // (a NaN or infinite coordinate fails a strict comparison)
    if (rule.has_fov) {
        const float az = (float)atan2((double)y, (double)x);
        if (!(rule.fov[0] < az && az < rule.fov[1])) return false;
        const float el = (float)atan2((double)z, (double)d);
        if (!(rule.fov[2] < el && el < rule.fov[3])) return false;
    }
    return true;
}

__global__ __launch_bounds__(kCompactThreads) void scan_flag_kernel(const float4 *__restrict__ raw, const uint32_t *__restrict__ raw_label,
                                                                    const int64_t *__restrict__ row_begin,
                                                                    const int64_t *__restrict__ row_count, int max_rows,
                                                                    const int32_t *__restrict__ lut, int lut_len, Rule rule,
                                                                    unsigned char *__restrict__ flags, int *__restrict__ tile_count,
                                                                    int tiles, int *__restrict__ err) {
    const int b = blockIdx.y, tile = blockIdx.x;
    const int n = pn2_clamped_rows(row_count, b, max_rows);
    const int64_t t0 = (int64_t)tile * kCompactTile;
    if (t0 >= n) return;                                            // (uniform over the workgroup)
    const int64_t base = row_begin[b] + t0, at = (int64_t)b * tiles + tile;
    bool unmapped = false;
    pn2_compact_flag_tile((int)(n - t0 < kCompactTile ? n - t0 : kCompactTile), flags + at * kCompactTile, tile_count + at, [&](int i) {
        if (raw_label != nullptr) {
            const uint32_t sem = raw_label[base + i] & 0xFFFFu;
            const int32_t c = sem < (uint32_t)lut_len ? lut[sem] : -1;
            if (c < 0) unmapped = true;                             // (the reference's dict lookup raises KeyError)
            if (c <= 0) return false;
        }
        return geometry_keeps(raw[base + i], rule);
    });
    if (err != nullptr && __any(unmapped) && (threadIdx.x & (PN2_WAVE - 1)) == 0) atomicOr(err, PN2_SCAN_ERR_CLASS);
}

__global__ __launch_bounds__(kCompactThreads) void scan_write_kernel(const float4 *__restrict__ raw, const uint32_t *__restrict__ raw_label,
                                                                     const int64_t *__restrict__ row_begin,
                                                                     const int64_t *__restrict__ row_count, int max_rows,
                                                                     const int32_t *__restrict__ lut,
                                                                     const unsigned char *__restrict__ flags,
                                                                     const int *__restrict__ tile_offset, int tiles,
                                                                     const int64_t *__restrict__ out_begin, float4 *__restrict__ out_points,
                                                                     int32_t *__restrict__ out_labels, int32_t *__restrict__ out_index) {
    const int b = blockIdx.y, tile = blockIdx.x;
    const int n = pn2_clamped_rows(row_count, b, max_rows);
    const int64_t t0 = (int64_t)tile * kCompactTile;
    if (t0 >= n) return;
    const int64_t base = row_begin[b] + t0, at = (int64_t)b * tiles + tile;
    const int64_t out0 = out_begin[b] + tile_offset[at];
    pn2_compact_write_tile(flags + at * kCompactTile, [&](int i, int rank) {
        const int64_t o = out0 + rank;
        out_points[o] = raw[base + i];
        if (out_labels != nullptr) out_labels[o] = raw_label != nullptr ? lut[raw_label[base + i] & 0xFFFFu] - 1 : 0;
        if (out_index != nullptr) out_index[o] = (int32_t)(t0 + i);
    });
}

inline bool shape_ok(int B, int64_t max_rows) { return B >= 1 && B <= 65535 && max_rows >= 0 && max_rows < (int64_t)1 << 31; }

// the workspace: the compaction's part alone
Pn2Compact scan_work(int B, int64_t max_rows, void *base, int64_t *bytes = nullptr) {
    Pn2Arena a(base);
    const Pn2Compact w = pn2_compact_take(a, B, max_rows);
    if (bytes != nullptr) *bytes = a.bytes();
    return w;
}

}  // namespace

extern "C" {

int64_t pn2_scan_filter_workspace_bytes(int B, int64_t max_rows) {
    int64_t bytes = PN2_EINVAL;
    if (shape_ok(B, max_rows)) scan_work(B, max_rows, nullptr, &bytes);
    return bytes;
}

int pn2_scan_filter(const float *raw, const uint32_t *raw_label, const int64_t *row_begin, const int64_t *row_count, int B,
                    int64_t max_rows, const int32_t *lut, int lut_len, const float *fov, const float *box, const int64_t *out_begin,
                    float *out_points, int32_t *out_labels, int32_t *out_index, int64_t *out_count, int *err, void *workspace,
                    pn2_stream_t stream) {
    PN2_CHECK_ARG(raw && row_begin && row_count && out_begin && out_points && out_count && workspace);
    PN2_CHECK_ARG(shape_ok(B, max_rows));
    PN2_CHECK_ARG(raw_label == nullptr || (lut != nullptr && lut_len >= 1));
    PN2_CHECK_ARG(pn2_aligned(raw, 16) && pn2_aligned(out_points, 16) && pn2_aligned(workspace, 16));       // rows move as 16-byte words
    Rule rule = {};
    if (fov != nullptr) {
        rule.has_fov = 1;
        for (int k = 0; k < 4; ++k) rule.fov[k] = fov[k];
    }
    if (box != nullptr) {
        rule.has_box = 1;
        for (int k = 0; k < 8; ++k) rule.box[k] = box[k];
    }
    const Pn2Compact w = scan_work(B, max_rows, workspace);
    const dim3 grid((unsigned)w.tiles, (unsigned)B);
    hipLaunchKernelGGL(scan_flag_kernel, grid, dim3(kCompactThreads), 0, pn2_s(stream), reinterpret_cast<const float4 *>(raw), raw_label,
                       row_begin, row_count, (int)max_rows, lut, lut_len, rule, w.flags, w.tile_count, w.tiles, err);
    hipLaunchKernelGGL(pn2_compact_offsets_kernel, dim3((unsigned)B), dim3(PN2_WAVE), 0, pn2_s(stream), row_count, (int)max_rows,
                       w.tile_count, w.tile_offset, w.tiles, out_count, err, PN2_SCAN_ERR_ROWS);
    hipLaunchKernelGGL(scan_write_kernel, grid, dim3(kCompactThreads), 0, pn2_s(stream), reinterpret_cast<const float4 *>(raw), raw_label,
                       row_begin, row_count, (int)max_rows, lut, w.flags, w.tile_offset, w.tiles, out_begin,
                       reinterpret_cast<float4 *>(out_points), out_labels, out_index);
    return pn2_launch_status();
}

}  // extern "C"
