// Lovasz-Softmax (Berman, Triki, Blaschko, CVPR 2018): the convex surrogate of mean IoU, on a segmented stable radix sort.
// The rule is stated in include/pn2.h (pn2_lovasz_fwd) and in numpy in tests/lovasz_ref.py.  The authors' formulation sorts once per
// class in a Python loop and reads two counts back per class; here one call sorts every (image, class) segment at once and nothing
// returns to the host, so forward and backward capture into a graph.
//
// A segment is the N = R / images rows of one image seen by one class: S = images * C segments of equal length.  Per element a
// 32-bit key (the float32 bits of the error e = |fg - p|, turned so that ascending key = descending e; NaN first; rows that take no
// part last) and a 32-bit payload (row inside the image, the foreground flag, the sign of p - fg).  Launches, a launch boundary is
// the only ordering between them, no workgroup waits on another, no atomic decides a position:
//   key pass        one thread per row: softmax, C keys and payloads, the probabilities, a per-workgroup "target out of range" flag;
//   4 x             per-tile histogram of one 8-bit digit | per (segment, digit) exclusive scan over the tiles (a wave per row of
//                   counts, 64 tiles a step) | scatter: the rank of an element among the equal digits of its tile from ballots and
//                   an LDS table in row order, so equal keys keep their order: a stable least-significant-digit sort;
//   foreground scan per-tile foreground count | the same row scan (its total is the segment's G) ;
//   finalise        per tile: F_k from the tile offset and ballots, c_k in fp64 from (k, F_k, G), dp scattered to [R, C], the tile's
//                   fp64 partial of e * c_k summed in a fixed tree;
//   reduce          one workgroup: tile partials per segment in a fixed order, the means, the NaN of an out-of-range target.
// Every sum across threads is an integer count or an fp64 sum of fixed shape: the outputs are byte-identical from run to run.
#include "compact.h"
#include "softmax_row.h"

namespace {

// Every pass runs compact.h's workgroup; the sort, scan and finalise passes take its tile: kCompactTile elements of one segment,
// element = round * kThreads + thread, so row order is (round, wave, lane): kCompactSegments 64-element runs.
constexpr int kThreads = kCompactThreads;
constexpr int kWaves = kCompactWaves;
constexpr int kRadix = 256;
static_assert(kRadix == kThreads, "one thread per digit value in the scatter pass");
constexpr int kMaxClasses = 64;
constexpr unsigned kKeyAbsent = 0xFFFFFFFFu;      // a row that takes no part: after every real key (real keys are <= 0x7FFFFFFF)
constexpr unsigned kFgBit = 0x80000000u, kNegBit = 0x40000000u, kRowMask = 0x3FFFFFFFu;

struct Work {                                     // the shape's counts and the parts of the workspace, each 16-byte aligned when the base is
    int64_t N, S, nt, bad_blocks;                 // rows per image, segments, tiles per segment, workgroups of the key pass
    unsigned *key[2], *pay[2];
    int *hist, *totals, *tile_fg, *G;
    double *partial, *seg_loss;
    int *bad;
    int64_t bytes;
};

Work lovasz_work(int64_t R, int C, int images, void *base) {
    Pn2Arena a(base);
    const int64_t N = R / images, S = (int64_t)images * C, nt = pn2_cdiv(N, kCompactTile), bad_blocks = pn2_cdiv(R, kThreads);
    return {N, S, nt, bad_blocks,
            {a.take<unsigned>(S * N), a.take<unsigned>(S * N)}, {a.take<unsigned>(S * N), a.take<unsigned>(S * N)},
            a.take<int>(S * kRadix * nt), a.take<int>(S * kRadix), a.take<int>(S * nt), a.take<int>(S),
            a.take<double>(S * nt), a.take<double>(S), a.take<int>(bad_blocks), a.bytes()};
}

// ------------------------------------------------------------------------------------------------------------------ key pass
// p of a row exactly as pn2_cross_entropy_bwd recomputes it (softmax_row.h): expf((x - max) - logf(sum))
template <int KC>
__device__ __forceinline__ void row_probabilities(const float *__restrict__ row, int64_t step, int C, int from_logits, float (&v)[KC]) {
    pn2_load_row_strided<KC>(row, step, C, v);
    if (!from_logits) return;
    const float logs = pn2_center_logsum<KC>(C, v);
#pragma unroll
    for (int c = 0; c < KC; ++c)
        if (c < C) v[c] = expf(v[c] - logs);
}

__device__ __forceinline__ int64_t row_base(int64_t r, int ld, int64_t inner, int C) {
    return inner == 0 ? r * ld : pn2_class_strided_base(r, inner, C);
}

template <int KC>
__global__ __launch_bounds__(kThreads) void key_kernel(const float *__restrict__ x, int ld, int64_t inner,
                                                       const int64_t *__restrict__ target, int64_t R, int C, int64_t N,
                                                       int64_t ignore_index, int from_logits, unsigned *__restrict__ keys,
                                                       unsigned *__restrict__ pays, float *__restrict__ prob,
                                                       int *__restrict__ bad_flags) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    int bad = 0;
    if (r < R) {
        float v[KC];
        row_probabilities<KC>(x + row_base(r, ld, inner, C), inner == 0 ? 1 : inner, C, from_logits, v);
        const int64_t t = target[r];
        const bool part = t != ignore_index && t >= 0 && t < C;
        bad = !part && t != ignore_index;
        const int64_t b = r / N;
        const unsigned n = (unsigned)(r - b * N);
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            if (c >= C) continue;
            if (prob != nullptr) prob[r * C + c] = v[c];
            unsigned key = kKeyAbsent, pay = n;
            if (part) {
                const float fg = c == (int)t ? 1.f : 0.f;
                const float d = v[c] - fg;
                const float e = fabsf(d);                                   // = fl32(|fg - p|)
                key = e != e ? 0u : 0x7FFFFFFFu - __float_as_uint(e);        // every NaN is one key: the largest error
                pay = n | (c == (int)t ? kFgBit : 0u) | (d < 0.f ? kNegBit : 0u);
            }
            const int64_t at = (b * C + c) * N + n;
            keys[at] = key;
            pays[at] = pay;
        }
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) bad_flags[blockIdx.x] = bad;
}

// ---------------------------------------------------------------------------------------------------------------------- sort
// counts of one digit in one tile -> hist[segment][digit][tile]
__global__ __launch_bounds__(kThreads) void hist_kernel(const unsigned *__restrict__ keys, int *__restrict__ hist, int64_t N, int nt,
                                                        int shift) {
    __shared__ int h[kRadix];
    const int64_t seg = blockIdx.x / nt;
    const int tile = (int)(blockIdx.x - seg * nt);
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t first = (int64_t)tile * kCompactTile;
#pragma unroll
    for (int r = 0; r < kCompactRounds; ++r) {
        const int64_t i = first + r * kThreads + threadIdx.x;
        if (i < N) atomicAdd(&h[(keys[seg * N + i] >> shift) & (kRadix - 1)], 1);      // a count: the same whatever the order
    }
    __syncthreads();
    hist[(seg * kRadix + threadIdx.x) * nt + tile] = h[threadIdx.x];
}

// One wave per row of nt counts: the row becomes its exclusive prefix sum, totals[row] its sum
__global__ __launch_bounds__(kThreads) void row_scan_kernel(int *__restrict__ data, int *__restrict__ totals, int64_t rows, int nt) {
    const int64_t row = (int64_t)blockIdx.x * kWaves + threadIdx.x / PN2_WAVE;
    if (row >= rows) return;                                             // uniform over the wave
    const int total = pn2_wave_row_excl_scan(data + row * nt, data + row * nt, nt);
    if ((threadIdx.x & (PN2_WAVE - 1)) == 0) totals[row] = total;
}

// element -> base of its digit in the segment + its digit's elements in earlier tiles + in earlier 64-runs of this tile + in
// earlier lanes of its run
__global__ __launch_bounds__(kThreads) void scatter_kernel(const unsigned *__restrict__ keys_in, const unsigned *__restrict__ pays_in,
                                                           unsigned *__restrict__ keys_out, unsigned *__restrict__ pays_out,
                                                           const int *__restrict__ offs, const int *__restrict__ totals, int64_t N,
                                                           int nt, int shift) {
    __shared__ int cnt[kCompactSegments * kRadix];
    __shared__ int base[kRadix];
    __shared__ int s_wave[kWaves];
    const int64_t seg = blockIdx.x / nt;
    const int tile = (int)(blockIdx.x - seg * nt);
    const int lane = threadIdx.x & (PN2_WAVE - 1), wave = threadIdx.x / PN2_WAVE;
    for (int i = threadIdx.x; i < kCompactSegments * kRadix; i += kThreads) cnt[i] = 0;
    const int before = pn2_block_excl_scan(totals[seg * kRadix + threadIdx.x], s_wave);
    base[threadIdx.x] = before + offs[(seg * kRadix + threadIdx.x) * nt + tile];
    __syncthreads();
    const int64_t first = (int64_t)tile * kCompactTile;
    unsigned key[kCompactRounds], pay[kCompactRounds];
    int rank[kCompactRounds];
    bool valid[kCompactRounds];
#pragma unroll
    for (int r = 0; r < kCompactRounds; ++r) {
        const int64_t i = first + r * kThreads + threadIdx.x;
        valid[r] = i < N;
        key[r] = valid[r] ? keys_in[seg * N + i] : 0u;
        pay[r] = valid[r] ? pays_in[seg * N + i] : 0u;
        const unsigned digit = (key[r] >> shift) & (kRadix - 1);
        unsigned long long same = __ballot(valid[r]);                   // the lanes of this run that hold the same digit
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool set = (digit >> bit) & 1u;
            const unsigned long long m = __ballot(set);
            same &= set ? m : ~m;
        }
        const unsigned long long below = same & ((1ull << lane) - 1ull);
        rank[r] = __popcll(below);
        if (valid[r] && below == 0ull) cnt[(r * kWaves + wave) * kRadix + digit] = __popcll(same);
    }
    __syncthreads();
    {
        int run = 0;                                                     // thread d: digit d's counts over the runs, in row order
#pragma unroll
        for (int s = 0; s < kCompactSegments; ++s) {
            const int v = cnt[s * kRadix + threadIdx.x];
            cnt[s * kRadix + threadIdx.x] = run;
            run += v;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kCompactRounds; ++r) {
        if (!valid[r]) continue;
        const unsigned digit = (key[r] >> shift) & (kRadix - 1);
        const int64_t pos = (int64_t)base[digit] + cnt[(r * kWaves + wave) * kRadix + digit] + rank[r];
        if (pos < N) {                                                   // (always: the counts are of these very keys)
            keys_out[seg * N + pos] = key[r];
            pays_out[seg * N + pos] = pay[r];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- scan and finalise
__global__ __launch_bounds__(kThreads) void fg_count_kernel(const unsigned *__restrict__ pays, int *__restrict__ tile_fg, int64_t N,
                                                            int nt) {
    const int64_t seg = blockIdx.x / nt;
    const int tile = (int)(blockIdx.x - seg * nt);
    const int64_t first = (int64_t)tile * kCompactTile;
    pn2_compact_count_tile(tile_fg + seg * nt + tile, [&](int i) { return first + i < N && (pays[seg * N + first + i] & kFgBit) != 0u; });
}

// is class c of image b counted, and how many of the image's classes are
__device__ __forceinline__ int counted_classes(const int *__restrict__ G, const int32_t *__restrict__ class_mask, int present_only,
                                               int64_t b, int C, int c, bool *mine) {
    int n = 0;
    *mine = false;
    for (int j = 0; j < C; ++j) {
        const bool on = (class_mask == nullptr || class_mask[j] != 0) && (!present_only || G[b * C + j] > 0);
        n += on ? 1 : 0;
        if (j == c) *mine = on;
    }
    return n;
}

__global__ __launch_bounds__(kThreads) void finalise_kernel(const unsigned *__restrict__ keys, const unsigned *__restrict__ pays,
                                                            const int *__restrict__ tile_off, const int *__restrict__ G, int64_t N,
                                                            int nt, int C, int images, const int32_t *__restrict__ class_mask,
                                                            int present_only, float *__restrict__ dp, double *__restrict__ partial) {
    __shared__ double s_sum[kWaves];
    const int64_t seg = blockIdx.x / nt;
    const int tile = (int)(blockIdx.x - seg * nt);
    const int64_t b = seg / C;
    const int c = (int)(seg - b * C);
    const int lane = threadIdx.x & (PN2_WAVE - 1), wave = threadIdx.x / PN2_WAVE;
    bool counted;
    const int ncounted = counted_classes(G, class_mask, present_only, b, C, c, &counted);
    const double w = counted ? 1.0 / ((double)ncounted * (double)images) : 0.0;
    const int64_t g = G[seg];
    const int64_t first = (int64_t)tile * kCompactTile;
    unsigned key[kCompactRounds], pay[kCompactRounds];
    int fg_before[kCompactRounds];                                      // foreground rows of the tile before this one
    bool valid[kCompactRounds], fg[kCompactRounds];
#pragma unroll
    for (int r = 0; r < kCompactRounds; ++r) {
        const int64_t i = first + r * kThreads + threadIdx.x;
        valid[r] = i < N;
        key[r] = valid[r] ? keys[seg * N + i] : kKeyAbsent;
        pay[r] = valid[r] ? pays[seg * N + i] : 0u;
        fg[r] = (pay[r] & kFgBit) != 0u;
    }
    pn2_compact_rank_tile(fg, fg_before);
    double sum = 0.0;
    const int before = tile_off[seg * nt + tile];
#pragma unroll
    for (int r = 0; r < kCompactRounds; ++r) {
        if (!valid[r]) continue;
        const unsigned n = pay[r] & kRowMask;
        float out = 0.f;
        if (key[r] != kKeyAbsent && counted) {
            const float e = __uint_as_float(key[r] == 0u ? 0x7FC00000u : 0x7FFFFFFFu - key[r]);
            const int64_t k = first + r * kThreads + threadIdx.x + 1;    // 1-based rank: rows that take no part sort behind every real one
            const int64_t Fp = before + fg_before[r];
            const int64_t F = Fp + (fg[r] ? 1 : 0);
            const double Jk = 1.0 - (double)(g - F) / (double)(g + k - F);
            const double Jp = k == 1 ? 0.0 : 1.0 - (double)(g - Fp) / (double)(g + (k - 1) - Fp);
            const double ck = Jk - Jp;
            sum += (double)e * ck;
            const double sg = (e == 0.f || e != e) ? 0.0 : ((pay[r] & kNegBit) ? -1.0 : 1.0);     // sgn(p - fg); sgn(0) = sgn(NaN) = 0
            out = (float)((w * ck) * sg);
        }
        if ((int64_t)n < N) dp[(b * N + n) * C + c] = out;              // (always: the payloads are a permutation of the rows)
    }
    sum = pn2_wave_sum_f64(sum);
    if (lane == 0) s_sum[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < kWaves; ++i) t += s_sum[i];
        partial[seg * nt + tile] = t;
    }
}

// One workgroup: segment losses (tile partials in a fixed order), the mean over an image's counted segments, the mean over all images
__global__ __launch_bounds__(kThreads) void reduce_kernel(const double *__restrict__ partial, double *__restrict__ seg_loss,
                                                          const int *__restrict__ G, int nt, int C, int images,
                                                          const int32_t *__restrict__ class_mask, int present_only,
                                                          const int *__restrict__ bad_flags, int64_t bad_blocks, float *__restrict__ loss) {
    __shared__ double tree[kThreads];
    const int64_t S = (int64_t)images * C;
    const int lane = threadIdx.x & (PN2_WAVE - 1);
    for (int64_t seg = threadIdx.x / PN2_WAVE; seg < S; seg += kWaves) {       // a wave per segment: lane L adds tiles L, L + 64, ...
        double l = 0.0;
        for (int t = lane; t < nt; t += PN2_WAVE) l += partial[seg * nt + t];
        l = pn2_wave_sum_f64(l);                                             // a fixed tree: the same sum on every lane, every run
        if (lane == 0) seg_loss[seg] = l;
    }
    int bad = 0;
    for (int64_t i = threadIdx.x; i < bad_blocks; i += kThreads) bad |= bad_flags[i];
    bad = __syncthreads_or(bad);                                         // (also orders the seg_loss stores before the loads below)
    double acc = 0.0;
    for (int64_t b = threadIdx.x; b < images; b += kThreads) {
        double l = 0.0;
        int n = 0;
        for (int c = 0; c < C; ++c) {
            const bool on = (class_mask == nullptr || class_mask[c] != 0) && (!present_only || G[b * C + c] > 0);
            if (on) { l += seg_loss[b * C + c]; ++n; }
        }
        if (n > 0) acc += l / (double)n;
    }
    tree[threadIdx.x] = acc;
    __syncthreads();
    for (int w = kThreads / 2; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) tree[threadIdx.x] += tree[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = bad ? __builtin_nanf("") : (float)(tree[0] / (double)images);
}

// ------------------------------------------------------------------------------------------------------------------ backward
// dx = g * p * (dp - sum_j p_j dp_j) (from_logits: p recomputed as the forward took it) or g * dp, in the input's layout
template <int KC>
__global__ __launch_bounds__(kThreads) void bwd_kernel(const float *__restrict__ x, int ld, int64_t inner, const float *__restrict__ dp,
                                                       int64_t R, int C, int from_logits, const float *__restrict__ grad_out,
                                                       float *__restrict__ dx) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= R) return;
    const int64_t base = row_base(r, ld, inner, C), step = inner == 0 ? 1 : inner;
    const float g = *grad_out;
    float d[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c)
        if (c < C) d[c] = dp[r * C + c];
    if (from_logits) {
        float p[KC];
        row_probabilities<KC>(x + base, step, C, 1, p);
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < KC; ++c)
            if (c < C) s += p[c] * d[c];
#pragma unroll
        for (int c = 0; c < KC; ++c)
            if (c < C) d[c] = g * (p[c] * (d[c] - s));
    } else {
#pragma unroll
        for (int c = 0; c < KC; ++c)
            if (c < C) d[c] = g * d[c];
    }
#pragma unroll
    for (int c = 0; c < KC; ++c)
        if (c < C) dx[base + c * step] = d[c];
}

int check_shape(int64_t R, int C, int images) {
    PN2_CHECK_ARG(R > 0 && C > 0 && C <= kMaxClasses && images > 0 && R % images == 0);
    PN2_CHECK_ARG(R / images <= (int64_t)kRowMask && R * C < (1LL << 36) && pn2_cdiv(R, kThreads) < (1LL << 31));
    const Work L = lovasz_work(R, C, images, nullptr);
    PN2_CHECK_ARG(L.S * L.nt < (1LL << 31) && L.S * kRadix < (1LL << 31));
    return PN2_OK;
}

int check_layout(int ld, int64_t inner, int64_t R, int C) {
    if (inner == 0) PN2_CHECK_ARG(ld >= C);
    else PN2_CHECK_ARG(inner > 0 && R % inner == 0);
    return PN2_OK;
}

}  // namespace

extern "C" {

int pn2_lovasz_tile_rows(void) { return kCompactTile; }

int64_t pn2_lovasz_workspace_bytes(int64_t R, int C, int images) {
    if (check_shape(R, C, images) != PN2_OK) return PN2_EINVAL;
    return lovasz_work(R, C, images, nullptr).bytes;
}

int pn2_lovasz_fwd(const float *x, int ld, int64_t inner, const int64_t *target, int64_t R, int C, int images, int64_t ignore_index,
                   int from_logits, const int32_t *class_mask, int present_only, void *workspace, float *dp, float *prob, float *loss,
                   pn2_stream_t stream) {
    PN2_CHECK_ARG(x && target && workspace && dp && loss && check_shape(R, C, images) == PN2_OK && check_layout(ld, inner, R, C) == PN2_OK);
    PN2_CHECK_ARG(pn2_aligned(workspace, 16) && pn2_aligned(x, 4) && pn2_aligned(dp, 4) && pn2_aligned(prob, 4) && pn2_aligned(loss, 4) &&
                  pn2_aligned(target, 8) && pn2_aligned(class_mask, 4));
    PN2_CHECK_ARG(images == 1 || inner == 0 || inner == R / images);     // class-strided: an image is one [C, inner] block
    const Work L = lovasz_work(R, C, images, workspace);
    hipStream_t s = pn2_s(stream);
    const int nt = (int)L.nt;
    const dim3 rows((unsigned)L.bad_blocks), tiles((unsigned)(L.S * L.nt)), block(kThreads);
#define PN2_LOVASZ_KEY(KC)                                                                                                          \
    hipLaunchKernelGGL(key_kernel<KC>, rows, block, 0, s, x, ld, inner, target, R, C, L.N, ignore_index, from_logits, L.key[0], L.pay[0], prob, L.bad)
    if (C <= 16) PN2_LOVASZ_KEY(16);
    else if (C <= 32) PN2_LOVASZ_KEY(32);
    else PN2_LOVASZ_KEY(64);
#undef PN2_LOVASZ_KEY
    for (int pass = 0; pass < 4; ++pass) {                               // 4 x 8 bits: the last pass leaves the result in key[0] / pay[0]
        const int in = pass & 1, out = in ^ 1, shift = 8 * pass;
        hipLaunchKernelGGL(hist_kernel, tiles, block, 0, s, L.key[in], L.hist, L.N, nt, shift);
        hipLaunchKernelGGL(row_scan_kernel, dim3((unsigned)pn2_cdiv(L.S * kRadix, kWaves)), block, 0, s, L.hist, L.totals, L.S * kRadix, nt);
        hipLaunchKernelGGL(scatter_kernel, tiles, block, 0, s, L.key[in], L.pay[in], L.key[out], L.pay[out], L.hist, L.totals, L.N, nt, shift);
    }
    hipLaunchKernelGGL(fg_count_kernel, tiles, block, 0, s, L.pay[0], L.tile_fg, L.N, nt);
    hipLaunchKernelGGL(row_scan_kernel, dim3((unsigned)pn2_cdiv(L.S, kWaves)), block, 0, s, L.tile_fg, L.G, L.S, nt);
    hipLaunchKernelGGL(finalise_kernel, tiles, block, 0, s, L.key[0], L.pay[0], L.tile_fg, L.G, L.N, nt, C, images, class_mask, present_only, dp,
                       L.partial);
    hipLaunchKernelGGL(reduce_kernel, dim3(1), block, 0, s, L.partial, L.seg_loss, L.G, nt, C, images, class_mask, present_only, L.bad,
                       L.bad_blocks, loss);
    return pn2_launch_status();
}

int pn2_lovasz_bwd(const float *x, int ld, int64_t inner, const float *dp, int64_t R, int C, int from_logits, const float *grad_out,
                   float *dx, pn2_stream_t stream) {
    PN2_CHECK_ARG(x && dp && grad_out && dx && check_shape(R, C, 1) == PN2_OK && check_layout(ld, inner, R, C) == PN2_OK);
    const dim3 rows((unsigned)pn2_cdiv(R, kThreads)), block(kThreads);
    hipStream_t s = pn2_s(stream);
#define PN2_LOVASZ_BWD(KC) hipLaunchKernelGGL(bwd_kernel<KC>, rows, block, 0, s, x, ld, inner, dp, R, C, from_logits, grad_out, dx)
    if (C <= 16) PN2_LOVASZ_BWD(16);
    else if (C <= 32) PN2_LOVASZ_BWD(32);
    else PN2_LOVASZ_BWD(64);
#undef PN2_LOVASZ_BWD
    return pn2_launch_status();
}

}  // extern "C"
