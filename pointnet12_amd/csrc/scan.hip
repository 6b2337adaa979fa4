// Scan ingest on the device: Semantic_KITTI_Utils.get (data_utils/kitti_utils.py:183-227) with points_basic_filter (:259-280)
// for a batch of raw scans that lie back to back in HBM -- the class map, the drop of class 0, the field-of-view / range-box
// test and the boolean-index compaction, without a host pass and with the kept count left in device memory.
//
//   pn2_scan_filter   three plain launches on the caller's stream, no workgroup ever waits on another:
//     scan_flag_kernel     one workgroup per tile of kScanTile rows: the rule of include/pn2.h per row, a one-byte flag per row and
//                          the tile's kept count (__ballot + popcount per wave, four waves summed through LDS);
//     scan_offsets_kernel  one wave per scan: exclusive prefix sum of its tiles' counts (64 tiles per step, shuffles), the scan's
//                          kept count, the "row_count above max_rows" bit;
//     scan_write_kernel    one workgroup per tile: rank inside the wave from the ballot, the sixteen 64-row segments of the tile
//                          ordered through LDS, every kept row moved as one 16-byte load and one 16-byte store.
//   Positions come from prefix sums alone (no atomics), so kept rows keep their scan order: the output is points[mask],
//   byte-identical from run to run.  A tile that starts at or beyond the device-side row count returns at once: a captured launch
//   sized by max_rows stays valid when the count changes.
//
// This file is built with -ffp-contract=off: d = sqrt((x*x + y*y) + z*z) is three separately rounded fp32 operations and a
// correctly rounded square root, as numpy's np.sqrt(x**2 + y**2 + z**2) is.  The two angles are fp64 atan2 values rounded to
// float32 (a definite rule; numpy's float32 arctan2 is not correctly rounded and differs between builds).
#include "pn2_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / PN2_WAVE;
constexpr int kRounds = PN2_SCAN_TILE / kThreads;                   // rows per thread; row = round * kThreads + thread
constexpr int kSegments = kRounds * kWaves;                         // 64-row segments of a tile, in row order
static_assert(PN2_SCAN_TILE % kThreads == 0 && kThreads % PN2_WAVE == 0, "a tile is a whole number of workgroup rounds");

struct Rule {
    float fov[4];                                                   // t0 < az < t1, t2 < el < t3
    float box[8];                                                   // x, y, z, d: lower, upper
    int has_fov, has_box;
};

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// rows of scan b this launch looks at: row_count[b] clamped to [0, max_rows]
__device__ __forceinline__ int clamped_rows(const int64_t *row_count, int b, int max_rows) {
    const int64_t n = row_count[b];
    return n < 0 ? 0 : (n > max_rows ? max_rows : (int)n);
}

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

__global__ __launch_bounds__(kThreads) void scan_flag_kernel(const float4 *__restrict__ raw, const uint32_t *__restrict__ raw_label,
                                                             const int64_t *__restrict__ row_begin,
                                                             const int64_t *__restrict__ row_count, int max_rows,
                                                             const int32_t *__restrict__ lut, int lut_len, Rule rule,
                                                             unsigned char *__restrict__ flags, int *__restrict__ tile_count,
                                                             int tiles, int *__restrict__ err) {
    __shared__ int s_count[kWaves];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int n = clamped_rows(row_count, b, max_rows);
    const int64_t t0 = (int64_t)tile * PN2_SCAN_TILE;
    if (t0 >= n) return;                                            // (uniform over the workgroup)
    const int64_t base = row_begin[b] + t0;
    const int left = (int)(n - t0 < PN2_SCAN_TILE ? n - t0 : PN2_SCAN_TILE);
    unsigned char *fl = flags + ((int64_t)b * tiles + tile) * PN2_SCAN_TILE;
    int kept = 0;
    bool unmapped = false;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const int i = r * kThreads + (int)threadIdx.x;
        bool keep = i < left;
        if (keep && raw_label != nullptr) {
            const uint32_t sem = raw_label[base + i] & 0xFFFFu;
            const int32_t c = sem < (uint32_t)lut_len ? lut[sem] : -1;
            if (c < 0) unmapped = true;                             // (the reference's dict lookup raises KeyError)
            keep = c > 0;
        }
        if (keep) keep = geometry_keeps(raw[base + i], rule);
        fl[i] = keep ? 1 : 0;                                       // every row of the tile, the ones beyond the scan as 0
        kept += __popcll(__ballot(keep));
    }
    const int lane = threadIdx.x & (PN2_WAVE - 1), wave = threadIdx.x / PN2_WAVE;
    if (err != nullptr && __any(unmapped) && lane == 0) atomicOr(err, PN2_SCAN_ERR_CLASS);
    if (lane == 0) s_count[wave] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) total += s_count[w];
        tile_count[(int64_t)b * tiles + tile] = total;
    }
}

__global__ __launch_bounds__(PN2_WAVE) void scan_offsets_kernel(const int64_t *__restrict__ row_count, int max_rows,
                                                                const int *__restrict__ tile_count, int *__restrict__ tile_offset,
                                                                int tiles, int64_t *__restrict__ out_count, int *__restrict__ err) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = clamped_rows(row_count, b, max_rows);
    const int active = (int)(((int64_t)n + PN2_SCAN_TILE - 1) / PN2_SCAN_TILE);       // <= tiles: n <= max_rows
    const int *cnt = tile_count + (int64_t)b * tiles;
    int *off = tile_offset + (int64_t)b * tiles;
    int carry = 0;                                                  // kept rows before this step: at most n < 2^31
    for (int first = 0; first < active; first += PN2_WAVE) {
        const int i = first + lane;
        const int v = i < active ? cnt[i] : 0;
        int incl = v;
#pragma unroll
        for (int d = 1; d < PN2_WAVE; d <<= 1) {
            const int up = __shfl_up(incl, d, PN2_WAVE);
            if (lane >= d) incl += up;
        }
        if (i < active) off[i] = carry + incl - v;
        carry += __shfl(incl, PN2_WAVE - 1, PN2_WAVE);
    }
    if (lane == 0) {
        out_count[b] = carry;
        if (err != nullptr && row_count[b] > max_rows) atomicOr(err, PN2_SCAN_ERR_ROWS);
    }
}

__global__ __launch_bounds__(kThreads) void scan_write_kernel(const float4 *__restrict__ raw, const uint32_t *__restrict__ raw_label,
                                                              const int64_t *__restrict__ row_begin,
                                                              const int64_t *__restrict__ row_count, int max_rows,
                                                              const int32_t *__restrict__ lut,
                                                              const unsigned char *__restrict__ flags,
                                                              const int *__restrict__ tile_offset, int tiles,
                                                              const int64_t *__restrict__ out_begin, float4 *__restrict__ out_points,
                                                              int32_t *__restrict__ out_labels, int32_t *__restrict__ out_index) {
    __shared__ int s_seg[kSegments];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int n = clamped_rows(row_count, b, max_rows);
    const int64_t t0 = (int64_t)tile * PN2_SCAN_TILE;
    if (t0 >= n) return;
    const int64_t base = row_begin[b] + t0;
    const unsigned char *fl = flags + ((int64_t)b * tiles + tile) * PN2_SCAN_TILE;
    const int lane = threadIdx.x & (PN2_WAVE - 1), wave = threadIdx.x / PN2_WAVE;
    bool keep[kRounds];
    int rank[kRounds];
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        keep[r] = fl[r * kThreads + (int)threadIdx.x] != 0;
        const unsigned long long m = __ballot(keep[r]);
        rank[r] = __popcll(m & ((1ull << lane) - 1ull));            // kept rows of this segment before this lane
        if (lane == 0) s_seg[r * kWaves + wave] = __popcll(m);
    }
    __syncthreads();
    const int64_t out0 = out_begin[b] + tile_offset[(int64_t)b * tiles + tile];
    int before = 0, seg = 0;                                        // kept rows of the tile in the segments before segment `seg`
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const int mine = r * kWaves + wave;
        for (; seg < mine; ++seg) before += s_seg[seg];
        if (keep[r]) {
            const int i = r * kThreads + (int)threadIdx.x;
            const int64_t o = out0 + before + rank[r];
            out_points[o] = raw[base + i];
            if (out_labels != nullptr) out_labels[o] = raw_label != nullptr ? lut[raw_label[base + i] & 0xFFFFu] - 1 : 0;
            if (out_index != nullptr) out_index[o] = (int32_t)(t0 + i);
        }
    }
}

inline int scan_tiles(int64_t max_rows) { return max_rows == 0 ? 1 : (int)pn2_cdiv(max_rows, PN2_SCAN_TILE); }
inline int64_t round16(int64_t v) { return (v + 15) / 16 * 16; }

}  // namespace

extern "C" {

int64_t pn2_scan_filter_workspace_bytes(int B, int64_t max_rows) {
    if (B < 1 || B > 65535 || max_rows < 0 || max_rows >= (int64_t)1 << 31) return PN2_EINVAL;
    const int64_t slots = (int64_t)B * scan_tiles(max_rows);
    return round16(slots * PN2_SCAN_TILE) + 2 * round16(slots * (int64_t)sizeof(int));     // flags, tile counts, tile offsets
}

int pn2_scan_filter(const float *raw, const uint32_t *raw_label, const int64_t *row_begin, const int64_t *row_count, int B,
                    int64_t max_rows, const int32_t *lut, int lut_len, const float *fov, const float *box, const int64_t *out_begin,
                    float *out_points, int32_t *out_labels, int32_t *out_index, int64_t *out_count, int *err, void *workspace,
                    pn2_stream_t stream) {
    PN2_CHECK_ARG(raw && row_begin && row_count && out_begin && out_points && out_count && workspace);
    PN2_CHECK_ARG(B >= 1 && B <= 65535 && max_rows >= 0 && max_rows < (int64_t)1 << 31);
    PN2_CHECK_ARG(raw_label == nullptr || (lut != nullptr && lut_len >= 1));
    PN2_CHECK_ARG(aligned16(raw) && aligned16(out_points) && aligned16(workspace));       // rows move as 16-byte words
    Rule rule = {};
    if (fov != nullptr) {
        rule.has_fov = 1;
        for (int k = 0; k < 4; ++k) rule.fov[k] = fov[k];
    }
    if (box != nullptr) {
        rule.has_box = 1;
        for (int k = 0; k < 8; ++k) rule.box[k] = box[k];
    }
    const int tiles = scan_tiles(max_rows);
    const int64_t slots = (int64_t)B * tiles;
    unsigned char *flags = static_cast<unsigned char *>(workspace);
    int *tile_count = reinterpret_cast<int *>(flags + round16(slots * PN2_SCAN_TILE));
    int *tile_offset = reinterpret_cast<int *>(reinterpret_cast<unsigned char *>(tile_count) + round16(slots * (int64_t)sizeof(int)));
    const dim3 grid((unsigned)tiles, (unsigned)B);
    hipLaunchKernelGGL(scan_flag_kernel, grid, dim3(kThreads), 0, pn2_s(stream), reinterpret_cast<const float4 *>(raw), raw_label,
                       row_begin, row_count, (int)max_rows, lut, lut_len, rule, flags, tile_count, tiles, err);
    hipLaunchKernelGGL(scan_offsets_kernel, dim3((unsigned)B), dim3(PN2_WAVE), 0, pn2_s(stream), row_count, (int)max_rows,
                       tile_count, tile_offset, tiles, out_count, err);
    hipLaunchKernelGGL(scan_write_kernel, grid, dim3(kThreads), 0, pn2_s(stream), reinterpret_cast<const float4 *>(raw), raw_label,
                       row_begin, row_count, (int)max_rows, lut, flags, tile_offset, tiles, out_begin,
                       reinterpret_cast<float4 *>(out_points), out_labels, out_index);
    return pn2_launch_status();
}

}  // extern "C"
