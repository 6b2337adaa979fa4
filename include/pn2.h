/*
 * pn2.h -- C ABI of libpn2_hip.so: the PointNet++ set-abstraction / feature-propagation
 * hot path as hand-written gfx950 (MI355X) HIP kernels.
 *
 * The reference (Jiang-Muyun/PointNet12) has no FFI: its hot path is 314 lines of ATen
 * calls in model/pointnet_util.py.  This library sits BELOW a Python mirror of that file
 * (pointnet12_amd/pointnet_util.py); every entry point names the reference lines whose
 * ATen op sequence it replaces.  INTEGRATION.md shows the ctypes binding a maintainer of
 * the reference would add to call these from the original file.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless it says "host"; tensors are dense row-major
 *     with the shapes given; float = IEEE fp32; indices = int64 (torch.long at the API);
 *   - the caller owns all memory (no allocation, no retained pointers); the only process-wide state is the option table
 *     below, changed by nothing but pn2_set_option() -- the library never reads the environment;
 *   - `stream` is a hipStream_t passed as void*; work is enqueued, never synchronised;
 *   - return value: PN2_OK (0) or a negative PN2_E* code (pn2_error_string() names it);
 *     launch errors are reported through hipGetLastError() as PN2_ELAUNCH;
 *   - results: index outputs are bit-identical to the reference's CPU results (the fp32
 *     expression forms are pinned in oracle/pn2_oracle.c); float outputs agree to 1e-5.
 */
#ifndef PN2_H
#define PN2_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PN2_ABI_VERSION 15

/* Per-channel fp64 reduction buffers ("stats", "red") are PN2_STAT_REPLICAS interleaved copies of
 * double[2*C] (sum, then second moment): workgroups add into copy (workgroup index % replicas) so the
 * same-address atomic queues stay short; pn2_bn_finalize / pn2_bn_bwd_coef sum the copies.  The caller
 * allocates and zeroes PN2_STAT_REPLICAS * 2 * C doubles. */
#define PN2_STAT_REPLICAS 8
#define PN2_DWX_REPLICAS 32   /* copies of the dWx partial block in pn2_group_affine_bwd_seg's scratch */

#define PN2_OK 0
#define PN2_OK_SPLIT 1            /* pn2_conv1x1_bwd_pair only: done, but issued as two launches (not an error) */
#define PN2_EINVAL (-1)     /* bad argument (null pointer, non-positive size, unsupported shape) */
#define PN2_ELAUNCH (-2)    /* hipLaunch / hipMemsetAsync failed */
#define PN2_EUNSUPPORTED (-3)

typedef void *pn2_stream_t;

/* Consumer-side BatchNorm (ABI 8).  The statistics -> affine block step of training-mode BatchNorm (pn2_bn_finalize) and the
 * reductions -> coefficients step of its backward (pn2_bn_bwd_coef) as a PROLOGUE of the first launch that reads the block,
 * instead of a launch of their own (one fused relu(bn(conv)) per layer in the reference: model/pointnet_util.py:195-197,
 * :252-255, :309-312).  The entry points that take a `const pn2_bn_lazy *` / `const pn2_bn_coef_lazy *` fill `affine` /
 * `coef` (which MUST be the very block passed as their in_affine / affine / coef argument) from the finished sums before
 * they read it; the block is valid for every later launch.  NULL: the block was already written.  Running statistics,
 * num_batches_tracked and dgamma / dbeta are updated exactly once per call. */
typedef struct pn2_bn_lazy {
    const double *stats;          /* replicated sums of the producing launch (PN2_STAT_REPLICAS x 2 x C doubles) */
    const float *gamma, *beta;    /* BatchNorm weight / bias, float[C] */
    float eps, momentum;
    float *running_mean, *running_var;      /* may be NULL */
    int64_t *num_batches_tracked;           /* may be NULL */
    float *affine;                /* float[4 * round4(C)], pad entries zero: filled */
    int64_t count;                /* rows the statistics were taken over */
    int C;
} pn2_bn_lazy;

typedef struct pn2_bn_coef_lazy {
    const double *red;            /* replicated reductions (sum dZ, sum dZ * yhat) of the producing launch */
    const float *gamma;
    const float *affine;          /* this layer's affine block */
    float *coef;                  /* float[4 * round4(C)]: filled */
    float *dgamma, *dbeta;        /* may be NULL */
    int accumulate;               /* != 0: dgamma / dbeta are added to */
    int64_t count;
    int C;
} pn2_bn_coef_lazy;

int pn2_version(void);
const char *pn2_error_string(int code);
/* Diagnostics (ABI 11): the kernel template instantiation the CALLING THREAD's most recent GEMM entry point enqueued, spelled as
 * rocprofv3 prints it ("(anonymous namespace)::split_bwd_res_kernel<4, 3, true, true>"), or NULL.  Thread-local; the launchers
 * store a pointer, nothing in the library reads it: bench.py prices every launch of its instrumented pass per KERNEL with it. */
const char *pn2_last_kernel(void);
void pn2_clear_last_kernel(void);

/* Dispatch / tuning options (ABI 10).  Which kernel family takes a layer, tile overrides, A/B switches of measured
 * experiments: one process-wide table of ints, every default the measured winner (the list with defaults and meanings:
 * PN2_OPTION_LIST in pointnet12_amd/csrc/pn2_common.h).  `name` is
 * the option's name with or without its "PN2_" prefix ("PN2_RING", "WIDE_MIN_ROWS", ...).  An option takes effect with the
 * next call; set options before work is enqueued from several threads.  pn2_option_name(i): name of option i, NULL past the
 * end (enumeration).  Unknown name: PN2_EINVAL.
 *
 * NUMERICS CONTRACT.  Every option but the two groups below changes results by fp32 summation order at most.  The exceptions
 * choose the ARITHMETIC a GEMM layer runs in, and are ON by default:
 *   SPLIT (with SPLIT_WGRAD, SPLIT_K256, SPLIT_NARROW, SPLIT_RES, SPLIT_MIN_ROWS_128, SPLIT_RES_MIN_TILES_128 selecting layers):
 *     1 = the long layers (from 65 536 rows) form every fp32 product from EXACT three-way bf16 splits of both operands
 *     (x = hi + mid + lo, 8 + 8 + 8 significand bits) as six v_mfma_f32_32x32x16_bf16 products accumulated in fp32; the three
 *     dropped cross terms are <= 2^-24 |a b| each.  Error against fp64: <= that of the sequential fp32 fma chain of
 *     v_mfma_f32_32x32x2_f32 it replaces (2.9e-6 vs 5.3e-6 at K = 128, profiles/r05_split_gemm_probe.txt), same 1e-5 contract.
 *     PRECONDITION: finite operands with |x| < 2^127 (bf16 rounds a larger |x| to inf and the residual becomes NaN where the
 *     fp32 pipe gives a finite product), and pieces below 2^-126 are flushed (the lo piece of |x| < 2^-110 is lost: relative
 *     error up to 2^-16 on such operands).  Activations, weights and gradients of a BatchNorm network sit 30 binades inside both.
 *     0 = v_mfma_f32_32x32x2_f32 everywhere (an exact fp32 fma chain per output element).
 *   POOL_CF: 2 (default) = a pooled last layer of 128 x 96 or 128 x 64 (1: 128 x 96 only; 0: off) never writes its pre-BN output; its backward is evaluated from the
 *     layer's input (pn2_conv1x1_bwd_cf: the same function, another rounding order; fp64-checked to 3e-6).
 * A caller that needs one arithmetic across library versions sets these explicitly. */
int pn2_set_option(const char *name, int value);
int pn2_get_option(const char *name, int *value);
const char *pn2_option_name(int index);

/* ------------------------------------------------------------------ geometry (index-exact) */

/* farthest_point_sample, model/pointnet_util.py:63-84 (the npoint-iteration Python loop).
 * xyz [B,N,3]; start [B] = the randint draw of :75 (host code owns the RNG);
 * out_idx [B,npoint].  work: caller scratch of pn2_fps_workspace_bytes(B,N,npoint) bytes (may be
 * NULL when that is 0; contents need not be initialised).  Distance form ((dx*dx+dy*dy)+dz*dz)
 * un-fused, argmax ties to the lowest index.  N <= 24576: one workgroup per cloud, cloud and running
 * distances in registers; larger clouds are spread over up to 16 cooperating workgroups each. */
int64_t pn2_fps_workspace_bytes(int B, int N, int npoint);
int pn2_fps(const float *xyz, int B, int N, const int64_t *start, int npoint, int64_t *out_idx,
            void *work, pn2_stream_t stream);

/* query_ball_point, model/pointnet_util.py:87-107 (dense [B,S,N] distance matrix + sort).
 * xyz [B,N,3], new_xyz [B,S,3], r2 = float32(radius**2); out_idx [B,S,nsample]: the first
 * nsample indices with !(d > r2) in ascending order, padded with the first; N everywhere
 * for an empty ball (the reference's tensor at :107). */
int pn2_ball_query(const float *xyz, const float *new_xyz, int B, int N, int S, float r2, int nsample,
                   int64_t *out_idx, pn2_stream_t stream);
/* The same query with caller scratch (`work`: pn2_ball_query_workspace_bytes(B, N, S) bytes, 4-byte aligned; 0 bytes / NULL:
 * identical to pn2_ball_query): on large clouds the centres are first put in spatial (Morton-cell) order so that the sixteen
 * centres a workgroup scans for have similar neighbour densities -- same out_idx, bit for bit. */
int64_t pn2_ball_query_workspace_bytes(int B, int N, int S);
int pn2_ball_query_ws(const float *xyz, const float *new_xyz, int B, int N, int S, float r2, int nsample, int64_t *out_idx,
                      void *work, pn2_stream_t stream);

/* square_distance, model/pointnet_util.py:19-40. src [B,S,3], dst [B,N,3] -> out [B,S,N]. */
int pn2_square_distance(const float *src, const float *dst, int B, int S, int N, float *out, pn2_stream_t stream);

/* 3-NN search + inverse-distance weights, model/pointnet_util.py:295-300 (dense matrix +
 * full sort + clamp 1e-10 + reciprocal + normalise).  xyz1 [B,N,3], xyz2 [B,S,3], S >= 3.
 * idx [B,N,3], dist [B,N,3] (raw, unclamped, ascending), weight [B,N,3]. Ties -> lower index. */
int pn2_three_nn(const float *xyz1, const float *xyz2, int B, int N, int S, int64_t *idx, float *dist,
                 float *weight, pn2_stream_t stream);

/* ------------------------------------------------------------------ gathers / scatters */

/* index_points, model/pointnet_util.py:43-60.  points [B,N,C], idx [B,M] -> out [B,M,C].
 * err (device int, may be NULL): set to 1 if any index is outside [0,N) (the reference raises
 * IndexError); offending rows are written as zeros. */
int pn2_gather_rows(const float *points, const int64_t *idx, int B, int N, int C, int M, float *out, int *err,
                    pn2_stream_t stream);
/* backward of the above: grad_points [B,N,C] += scatter of grad_out [B,M,C] (caller zeroes). */
int pn2_gather_rows_bwd(const float *grad_out, const int64_t *idx, int B, int N, int C, int M, float *grad_points,
                        pn2_stream_t stream);

/* Grouping of sample_and_group (:127-133) and of the MSG loop (:243-251): gather K
 * neighbours, subtract the centroid from xyz, concatenate with the D features.
 * xyz [B,N,3], points [B,N,D] or NULL (D = 0), new_xyz [B,S,3], idx [B,S,K].
 * out [B*S*K, ld] position-major rows, ld >= 3+D and a multiple of 4; row = [xyz-c, feat] if xyz_first (SSG, :131)
 * else [feat, xyz-c] (MSG, :247); columns 3+D..ld-1 are zero.  new_xyz == NULL means
 * "do not centre" (sample_and_group_all, :140-157, with idx = arange). */
int pn2_group(const float *xyz, const float *points, const float *new_xyz, const int64_t *idx, int B, int N, int S,
              int K, int D, int xyz_first, int ld, float *out, int *err, pn2_stream_t stream);
/* backward: grad_points [B,N,D] += feature columns of grad_rows [B*S*K, ld] (caller zeroes). */
int pn2_group_bwd(const float *grad_rows, const int64_t *idx, int B, int N, int S, int K, int D, int xyz_first,
                  int ld, float *grad_points, pn2_stream_t stream);

/* pn2_group + the FIRST conv of a shared MLP in one launch, for narrow first layers (3 + D <= 12 input channels, C_out 32
 * or 64, B*S*K a multiple of 64; otherwise PN2_EUNSUPPORTED and nothing is launched): X [B*S*K, ldx] receives the grouped
 * rows exactly as pn2_group writes them (the backward's weight gradient reads them), Y [B*S*K, ldy] = X W^T + bias with
 * W [C_out, 3 + D] as stored (pitch ldw), stats (may be NULL) the per-channel sums like pn2_conv1x1_fwd.
 * Refused as well: ldx > 12, idx or new_xyz NULL.  Every column of X up to the pitch is written: the centred coordinates are
 * fp32(xyz_j - c_s), one rounding, the features copies, the pad columns [3 + D, ldx) zero.  Of Y only the columns [0, C_out)
 * are written; [C_out, ldy) are left alone.  Y has the same bits with and without stats.
 * model/pointnet_util.py:127-131 + :197, :243-247 + :254. */
int pn2_group_conv_fwd(const float *xyz, const float *points, const float *new_xyz, const int64_t *idx, int B, int N, int S,
                       int K, int D, int xyz_first, const float *W, int ldw, const float *bias, float *X, int ldx, float *Y, int ldy,
                       int C_out, double *stats, pn2_stream_t stream);

/* Factorised first MLP layer of a set-abstraction level (replaces gather + cat + the first 1x1 conv,
 * model/pointnet_util.py:127-131,:197 / :243-247,:254, for that layer only):
 *   Y[p, c] = Zf[b, idx[p], c] + sum_a Wx[c, a] * (xyz[b, idx[p], a] - new_xyz[b, s, a]),  p = (b, s, k)
 * with Zf [B*N, ldz] = W_f f + bias precomputed per SOURCE point (one small pn2_conv1x1_fwd) and
 * Wx [C, 3] (row pitch ldwx >= 3) the xyz columns of the layer's weight -- it may point into the full
 * [C, 3+D] weight.  stats as in pn2_conv1x1_fwd (double[2*C], may be NULL). */
int pn2_group_affine_fwd(const float *Zf, int ldz, const float *xyz, const float *new_xyz, const int64_t *idx,
                         const float *Wx, int ldwx, int B, int N, int S, int K, int C, float *Y, int ldy,
                         double *stats, pn2_stream_t stream);
/* backward: dY = c0*dZ + q1*(y-mean) + q0 (coef from pn2_bn_bwd_coef) is scattered to the source points,
 * G[b*N + idx[p], :] += dY[p, :] (G [B*N, ldg], caller zeroes), and dWx[c, a] += dY[p, c] * (xyz - centre)[a]
 * (dWx [C, 3] with row pitch ldwx >= 3 -- it may point at the xyz columns of the full weight gradient --
 * caller zeroes or accumulates). */
int pn2_group_affine_bwd(const float *dZ, int ldz, const float *Y, int ldy, const float *coef, const float *xyz,
                         const float *new_xyz, const int64_t *idx, int B, int N, int S, int K, int C, float *G, int ldg,
                         float *dWx, int ldwx, pn2_stream_t stream);

/* Inverse-distance interpolation, model/pointnet_util.py:301: out[b,n,col0+c] =
 * ((p2[i0,c]*w0 + p2[i1,c]*w1) + p2[i2,c]*w2).  points2 [B,S,D]; out rows of pitch ld
 * (so the result lands directly inside the concatenated FP input, :305).  zero_tail != 0: the columns
 * col0+D .. ld-1 of every row are cleared as well (the pad lanes of a float4-pitched row; nobody pre-clears it).
 * points1 != NULL ([B,N,col0] contiguous): the same launch copies it into columns 0..col0-1, i.e. the whole
 * cat([points1, interpolated], -1) of :305 is one kernel. */
int pn2_three_interp(const float *points2, const int64_t *idx, const float *weight, int B, int N, int S, int D,
                     float *out, int ld, int col0, int zero_tail, const float *points1, pn2_stream_t stream);
/* backward: grad_points2 [B,S,D] += w_k * grad_out[b,n,col0+c] (caller zeroes).  S == 1 (the repeat branch of :292-293: every
 * index is 0, idx is not read): a deterministic column sum, STORED into grad_points2. */
int pn2_three_interp_bwd(const float *grad_out, int ld, int col0, const int64_t *idx, const float *weight, int B,
                         int N, int S, int D, float *grad_points2, pn2_stream_t stream);

/* Strided 2-D copy: dst[r, dcol0 + c] = src[r, scol0 + c], r < rows, c < cols (the cat of :305,
 * and its backward split). */
int pn2_copy_cols(const float *src, int lds, int scol0, float *dst, int ldd, int dcol0, int64_t rows, int cols,
                  pn2_stream_t stream);

/* ------------------------------------------------------------------ shared MLP (1x1 conv + BN + ReLU [+ max])
 *
 * Position-major activations: one grouped position per row, P = B*S*K rows (B*N for FP).
 * Replaces nn.Conv2d/Conv1d(k=1) + nn.BatchNorm2d/1d + F.relu (+ torch.max over K),
 * model/pointnet_util.py:194-199, :251-256, :309-312, and their autograd.
 *
 * Per-channel "affine" blocks are float[4*C] arrays written by pn2_bn_finalize:
 *   [0..C) mean   [C..2C) scale = gamma*invstd   [2C..3C) beta   [3C..4C) invstd
 * and relu((y-mean)*scale+beta) is applied on the fly wherever a pre-BN tensor is consumed.
 */

/* Y[P,N] = act(X)[P,K] * W[N,K]^T + bias.  X has row pitch ldx (>= round4(K), multiple of 4, pad
 * columns zero).  W is the Conv weight [N = C_out, K = C_in] as nn.Conv1d/2d stores it, row pitch
 * ldw >= K floats: no padding or alignment is required (16-byte aligned rows with K % 4 == 0 are read as
 * float4, anything else -- a C_in of 9 or 137, or the feature columns sliced out of a [C_out, 3+D]
 * weight -- with guarded scalar loads).  A 16-byte aligned W with ldw % 4 == 0 and ldw >= round4(K) is read as float4
 * too, the last quad of a row included: its pad entries [K, round4(K)) MUST then be zero (the host side hands over such a
 * padded copy of the 137-column weight of fp1's first layer: 38.5 -> 30.5 us at 65 536 rows).  Y pitch ldy (multiple of 4, >= round4(N); pad lanes are
 * written as zeros).  in_affine: NULL (X is used as is) or the affine block (4*ldx floats) of
 * the layer that produced X.  stats: NULL or a replicated double[2*N] block (see PN2_STAT_REPLICAS; caller zeroes) receiving
 * sum(y) and sum(y*y) per output channel over the P rows (training-mode BN statistics).  P < 2^31 rows for the three conv1x1 entry points (PN2_EINVAL otherwise). */
int pn2_conv1x1_fwd(const float *X, int ldx, const float *in_affine, const float *W, int ldw, const float *bias,
                    float *Y, int ldy, int64_t P, int K, int N, double *stats, const pn2_bn_lazy *in_lazy,
                    pn2_stream_t stream);

/* BatchNorm statistics -> affine block.  training != 0: mean/var (biased) from stats/P,
 * running_mean/var (may be NULL) updated with `momentum` and the unbiased variance,
 * *num_batches_tracked (may be NULL) incremented.  training == 0: running statistics are used. */
int pn2_bn_finalize(const double *stats, int64_t P, int C, const float *gamma, const float *beta, float eps,
                    float momentum, int training, float *running_mean, float *running_var,
                    int64_t *num_batches_tracked, float *affine, pn2_stream_t stream);

/* pn2_conv1x1_fwd for the LAST layer of a pooled shared MLP in training mode (model/pointnet_util.py:194-199 / :251-256: the
 * conv whose BN + ReLU output is max-reduced over the Kpool rows of a group), weight-resident kernel only: besides Y and the
 * statistics it records, per group and channel, the extreme pre-BN value -- the largest, or the smallest where gamma (this
 * layer's BatchNorm weight, float[C_out]) is negative -- and the first row attaining it into pool_ws (16-byte aligned
 * float[2 * (P / Kpool) * C_out]: {value, row as int32} pairs).  BN + ReLU is monotone per channel with the sign of gamma,
 * so pn2_bn_pool_select turns these into max_k relu(bn(y_k)) exactly once the affine block exists, and the pass over Y of
 * pn2_bn_relu_max is not needed.  Returns PN2_EUNSUPPORTED (nothing launched) when the shape is outside the resident kernels
 * (see pn2_res_supported; also needs P % 32 == 0, Kpool == 16 or Kpool % 32 == 0): call pn2_conv1x1_fwd + pn2_bn_relu_max
 * then. */
/* Y == NULL (ABI 11): the pre-BN output is not written at all -- statistics and extrema only.  Taken by the bf16-pipe forms of the
 * forward alone (PN2_EUNSUPPORTED otherwise: call again with a Y); the layer's backward then runs on the layer's INPUT:
 * pn2_pool_bwd_reduce_rec + pn2_conv1x1_bwd_cf below, where pn2_conv1x1_bwd_cf_supported() says so. */
int pn2_conv1x1_fwd_pool(const float *X, int ldx, const float *in_affine, const float *W, int ldw, const float *bias, float *Y,
                         int ldy, int64_t P, int K, int N, double *stats, int Kpool, const float *gamma, float *pool_ws,
                         const pn2_bn_lazy *in_lazy, pn2_stream_t stream);
/* out[g,c] = relu(bn(v)) of the recorded extreme value, arg[g,c] = its row (same outputs as pn2_bn_relu_max up to which of
 * several rows with EQUAL post-BN value is named; a channel whose scale is exactly 0 -- BatchNorm weight 0: every row gives
 * relu(beta) -- names row 0, as torch.max of an all-equal group does).  C % 32 == 0, ldo == C. */
int pn2_bn_pool_select(const float *pool_ws, const float *affine, int64_t G, int C, float *out, int ldo, int32_t *arg,
                       const pn2_bn_lazy *lazy, pn2_stream_t stream);

/* out[g,c] = max_k relu(bn(Y[g*K+k, c])), arg[g,c] = first k attaining it (K = 1: plain
 * BN+ReLU, arg may be NULL).  Y pitch ldy, out / arg pitch ldo: both multiples of 4 and >= round4(C)
 * (rows are moved as float4; the pad columns of out / arg are written too, from the zero pad of `affine`). */
int pn2_bn_relu_max(const float *Y, int ldy, const float *affine, int64_t G, int K, int C, float *out, int ldo,
                    int32_t *arg, const pn2_bn_lazy *lazy, pn2_stream_t stream);

/* Backward, last layer after max-pool: dZp[g,c] = out[g,c] > 0 ? dOut[g,c] : 0 (pitch ldo, pad lanes zero),
 * red[0..C) = sum dZ, red[C..2C) = sum dZ*yhat with dZ[g*K+k,c] = (k == arg[g,c]) ? dZp[g,c] : 0.
 * red is double[2*C], caller zeroes.
 * PRECONDITION on `out` (round 4): it must be the pooled output THIS affine block produced, bit for bit --
 * out[g,c] = max(fma(Y[(g*K + arg[g,c]), c] - mean, scale, beta), 0), what pn2_bn_relu_max / pn2_bn_pool_select write.
 * Where |gamma| >= (1 + |beta|) / 4 the kernels take yhat of a positive output from it, yhat = (out - beta) / gamma (error
 * eps * |out| / |gamma|: no gather of Y, one 64-byte sector per element); elsewhere (small or zero gamma) from Y as before.  An
 * `out` from another path (an eval-mode fold, a post-processed slice) gives wrong d gamma / q1.  Y must be non-NULL either way.
 * Both branches and both signs of gamma are held to an fp64 evaluation by tests/test_mlp_gpu.py
 * (test_shared_mlp_negative_and_zero_gamma). */
int pn2_pool_bwd_reduce(const float *dOut, int ldo, const float *out, const int32_t *arg, const float *Y, int ldy,
                        const float *affine, int64_t G, int K, int C, float *dZp, double *red,
                        pn2_stream_t stream);
/* The same with the incoming gradient at a pitch of its own (ld_dout >= C, any alignment): a column slice of a wider gradient
 * matrix -- what autograd hands a branch of a concatenated output -- is read in place instead of being copied out first. */
int pn2_pool_bwd_reduce_ld(const float *dOut, int ld_dout, const float *out, int ldo, const int32_t *arg, const float *Y, int ldy,
                           const float *affine, int64_t G, int K, int C, float *dZp, double *red, pn2_stream_t stream);
/* pn2_pool_bwd_reduce_ld for a pooled last layer whose pre-BN output was never written (pn2_conv1x1_fwd_pool with Y == NULL): the
 * value at the recorded row comes from pool_ws (the {value, row} records of that forward; `out` / `arg` from pn2_bn_pool_select of
 * the same records) -- exact for every gamma, no gather.  A channel whose folded scale is exactly 0 routes to row 0 of its group,
 * whose value the record does not hold: recomputed from the layer's input, y = bias[c] + W[c, :] . relu(bn(prev_Y[g K, :]))
 * (W [C, C_in] pitch ldw, prev_Y pitch ld_prev with its affine block of pitch round4(C_in)).  Same outputs as
 * pn2_pool_bwd_reduce_ld. */
int pn2_pool_bwd_reduce_rec(const float *dOut, int ld_dout, const float *out, int ldo, const int32_t *arg, const float *pool_ws,
                            const float *affine, int64_t G, int K, int C, float *dZp, double *red, const float *W, int ldw,
                            const float *bias, const float *prev_Y, int ld_prev, const float *prev_affine, int C_in,
                            pn2_stream_t stream);
/* Backward, dense (FP) last layer: dZ = dOut * (out > 0) written to dZ [P, ldz] (its pad columns
 * C .. round4(C)-1 are written as zeros); same reductions, same precondition on `out` (= max(fma(Y - mean, scale, beta), 0)). */
int pn2_relu_bwd_reduce(const float *dOut, int ldo, const float *out, const float *Y, int ldy, const float *affine,
                        int64_t P, int C, float *dZ, int ldz, double *red, pn2_stream_t stream);

/* Per-channel BN-backward coefficients from the reductions: coef float[4*C] =
 * [c0 = gamma*invstd, q1 = -c0*invstd*red1/P, q0 = -c0*red0/P, mean]; dgamma = red1, dbeta = red0.
 * dY = c0*dZ + q1*(y-mean) + q0.  use_batch_stats == 0 (eval-mode BN): q1 = q0 = 0.
 * accumulate != 0: dgamma/dbeta are added to (they alias existing .grad storage) instead of overwritten. */
int pn2_bn_bwd_coef(const double *red, int64_t P, int C, const float *gamma, const float *affine,
                    int use_batch_stats, float *coef, float *dgamma, float *dbeta, int accumulate, pn2_stream_t stream);

/* dgrad: dXact[P,N] = dY[P,K] * W[K,N] with dY formed on the fly from (dZ or the pooled
 * pair dOut/arg, Y, coef); K = C_l, N = C_{l-1}.  W is the SAME Conv weight [C_l, C_{l-1}] the forward
 * read (row pitch ldw >= N, no padding / alignment requirement; a 16-byte aligned W with ldw % 4 == 0 and ldw >= round4(N)
 * is read in whole quads and its pad entries [N, round4(N)) MUST be zero): the kernel reads it "down the columns",
 * no transposed copy exists.  dXout pitch ldxo (multiple of 4, >= round4(N); pad lanes written as zeros).
 *   dZ != NULL: dense dZ [P, ldz];  dZ == NULL: pooled form (dZp [G,ldo] from pn2_pool_bwd_reduce, arg, Kpool).
 * Epilogue, prev_Y != NULL: dZprev = dXact * (bn_relu(prev_Y) > 0) -> dXout, and
 *   prev_red (double[2*N], caller zeroes) += sum dZprev, sum dZprev*yhat_prev;
 * prev_Y == NULL (first layer): dXout = dXact. */
int pn2_conv1x1_dgrad(const float *dZ, int ldz, const float *dZp, int ldo, const int32_t *arg,
                      int Kpool, const float *Y, int ldy, const float *coef, const float *W, int ldw,
                      const float *prev_Y, int ld_prev, const float *prev_affine, float *dXout, int ldxo,
                      double *prev_red, int64_t P, int K, int N, const pn2_bn_coef_lazy *coef_lazy,
                      pn2_stream_t stream);

/* wgrad: dW[M,N] (pitch lddw, caller zeroes) += sum_p dY[p,m] * Xact[p,n]; M = C_l, N = C_{l-1}.
 * dY formed as in dgrad; Xact = bn_relu(prev_Y) when prev_affine != NULL, else X as is.
 * dbias (may be NULL, caller zeroes) += sum_p dY[p,m]. */
int pn2_conv1x1_wgrad(const float *dZ, int ldz, const float *dZp, int ldo, const int32_t *arg,
                      int Kpool, const float *Y, int ldy, const float *coef, const float *X, int ldx,
                      const float *x_affine, float *dW, int lddw, float *dbias, int64_t P, int M, int N,
                      const pn2_bn_coef_lazy *coef_lazy, pn2_stream_t stream);

/* pn2_conv1x1_wgrad with caller scratch (ABI 8): where pn2_conv1x1_wgrad_workspace_bytes(P, M, N, pooled) is > 0 and `workspace`
 * (16-byte aligned, that many bytes, contents irrelevant) is given, the full-tile kernel stores every workgroup's partial dW as
 * plain stores and a second small launch adds the slabs into dW (one atomic per element instead of one per workgroup and
 * element).  workspace == NULL or a query result of 0: exactly pn2_conv1x1_wgrad. */
int64_t pn2_conv1x1_wgrad_workspace_bytes(int64_t P, int M, int N, int pooled);
int pn2_conv1x1_wgrad_ws(const float *dZ, int ldz, const float *dZp, int ldo, const int32_t *arg,
                         int Kpool, const float *Y, int ldy, const float *coef, const float *X, int ldx,
                         const float *x_affine, float *dW, int lddw, float *dbias, int64_t P, int M, int N,
                         const pn2_bn_coef_lazy *coef_lazy, float *workspace, pn2_stream_t stream);

/* Weight gradient of a FIRST layer (C_in = N <= 15, C_out = M a multiple of 16, <= 128) whose data gradient nobody needs, from dZ
 * and the input rows alone (ABI 9).  The BatchNorm-backward terms of dY = c0*dZ + q1*(y - mean) + q0 (model/pointnet_util.py:195-197,
 * backward) are linear in sums the forward already fixed: with s = sum_p x_p, S = sum_p x_p x_p^T and y_p = W x_p + b,
 *     dW[c][j] += c0[c] * sum_p dZ[p,c] x[p,j] + q1[c] * ((W S)[c][j] + (b[c] - mean[c]) * s[j]) + q0[c] * s[j]
 * -- Y is never read (half the bytes of pn2_conv1x1_wgrad on these layers); s and S are accumulated by the same pass, in fp64 from
 * the first product on (the mean of x cancels between W S and (b - mean) s^T: an error of S is amplified by mean^2 / variance of
 * the input columns), and the closed-form part is added once, by the workgroup that finishes last.  Only the columns [0, N) of X,
 * W and dW and [0, M) of dZ are touched, whatever the pitches hold behind them.  `coef` as for pn2_conv1x1_wgrad
 * (rows c0, q1, q0, mean of pitch round4(M); realised from `coef_lazy` when given); W [M, N] (pitch ldw) and bias [M] are the
 * layer's parameters; `scratch`: pn2_conv1x1_wgrad_cf_scratch_bytes() bytes, 16-byte aligned, ZEROED by the caller (left dirty).
 * dZ == NULL (ABI 11): sum_p dZ[p,c] x[p,j] is already in `scratch` -- pn2_conv1x1_bwd_first of the NEXT layer added it there --
 * and this call takes the input's moments and finishes.
 * PN2_EUNSUPPORTED for other shapes: use pn2_conv1x1_wgrad. */
int64_t pn2_conv1x1_wgrad_cf_scratch_bytes(void);
int pn2_conv1x1_wgrad_cf(const float *dZ, int ldz, const float *coef, const float *X, int ldx, const float *W, int ldw,
                         const float *bias, void *scratch, float *dW, int lddw, int64_t P, int M, int N,
                         const pn2_bn_coef_lazy *coef_lazy, pn2_stream_t stream);

/* pn2_conv1x1_dgrad followed by pn2_conv1x1_wgrad of ONE layer (same dZ / pooled pair, Y, coef; X = the layer's input, i.e.
 * prev_Y wherever there is a previous layer, with x_affine = prev_affine) as one call: on the few-row and mid-size layers
 * (sa3 / sa4 / FP stacks, P up to 64 k rows) both kernel bodies share ONE launch -- the first workgroups of the grid compute
 * dX, the rest dW -- so neither leaves half of the chip idle and the chain is one launch shorter; elsewhere the two
 * launches are issued one after the other and the call returns PN2_OK_SPLIT (1) instead of PN2_OK.  Results are those of the
 * two separate calls. */
int pn2_conv1x1_bwd_pair(const float *dZ, int ldz, const float *dZp, int ldo, const int32_t *arg, int Kpool, const float *Y,
                         int ldy, const float *coef, const float *W, int ldw, const float *prev_Y, int ld_prev,
                         const float *prev_affine, float *dXout, int ldxo, double *prev_red, const float *X, int ldx,
                         const float *x_affine, float *dW, int lddw, int64_t P, int C_out, int C_in,
                         const pn2_bn_coef_lazy *coef_lazy, pn2_stream_t stream);

/* pn2_conv1x1_bwd of the LAST layer of a pooled shared MLP (model/pointnet_util.py:197-199, :254-256: conv + BN + ReLU + max over
 * Kpool rows) WITHOUT that layer's pre-BN output (ABI 11).  dZ is sparse there (one row per group and channel: dZp / arg as
 * pn2_pool_bwd_reduce_rec wrote them) and the dense part of dY = c0 dZ + q1 (y - mean) + q0 is affine in y = W x + b, hence in the
 * layer's input x = relu(bn(prev_Y)), which the pass reads anyway:
 *     dXout = ([D | X] [diag(c0) W ; W^T diag(q1) W] + (q1 (b - mean) + q0)^T W) masked by the previous ReLU, reductions into prev_red;
 *     dW   += c0 o (D^T X) + q1 o (W (X^T X) + (b - mean) (1^T X)) + q0 (1^T X)
 * -- the same function of the same inputs as pn2_conv1x1_bwd (fp32 rounding differs: tests/test_mlp_gpu.py holds both to fp64),
 * 4 P (2 C_in) bytes instead of 4 P (C_out + 2 C_in), and the forward writes no Y (pn2_conv1x1_fwd_pool with Y == NULL).
 * Partial products leave as one slab per workgroup and are summed in a fixed order: dW is run-to-run identical.
 * bias: the conv bias [C_out].  scratch: pn2_conv1x1_bwd_cf_scratch_bytes(C_out, C_in) bytes, 256-byte aligned, contents need
 * not be initialised.  Of dZp / arg only the columns [0, C_out) are read, whatever the pitch ldo holds behind them (arg's pad may
 * be garbage); dXout (pitch ldxo >= C_in, any) is written in [0, C_in) only.  Every row count P % Kpool == 0 from the threshold on
 * is taken: one 32-row chunk per workgroup up to min(CUs, 256) workgroups, round-robin beyond.
 * Training-mode BatchNorm, prev_affine != NULL.  pn2_conv1x1_bwd_cf_supported(): 1 where the call runs
 * (128 x 96 and 128 x 64 with Kpool a power of two >= 32, from pn2_res_supported()'s row count on, library options SPLIT /
 * SPLIT_RES / POOL_CF on); PN2_EUNSUPPORTED otherwise. */
int pn2_conv1x1_bwd_cf_supported(int64_t P, int C_out, int C_in, int Kpool);
int64_t pn2_conv1x1_bwd_cf_scratch_bytes(int C_out, int C_in);
int pn2_conv1x1_bwd_cf(const float *dZp, int ldo, const int32_t *arg, int Kpool, const float *coef, const float *W, int ldw,
                       const float *bias, const float *prev_Y, int ld_prev, const float *prev_affine, float *dXout, int ldxo,
                       double *prev_red, float *dW, int lddw, int64_t P, int C_out, int C_in,
                       const pn2_bn_coef_lazy *coef_lazy, float *scratch, pn2_stream_t stream);

/* pn2_conv1x1_bwd of a layer whose INPUT is the output of a FIRST layer with a narrow input X0 (N0 <= 12 columns: the grouped
 * 3 + D rows of sa1; model/pointnet_util.py:127-131 feeding :195-197 / :252-255) when nobody needs a gradient with respect to X0
 * (ABI 11).  The masked dX of this call IS that first layer's dZ; its backward (pn2_conv1x1_wgrad_cf: BatchNorm terms in closed
 * form) needs only sum_p dZ[p, c] X0[p, j] from it, which this call forms from its dX tiles and adds into THAT call's scratch
 * (cf_scratch: pn2_conv1x1_wgrad_cf_scratch_bytes() bytes, zeroed by the caller, then handed to pn2_conv1x1_wgrad_cf with
 * dZ == NULL) -- dX itself is never written.  dense dZ, prev_affine / prev_red required (training-mode BatchNorm), X0 16-byte
 * aligned with pitch ld0 >= 12, ld0 % 4 == 0 (pad columns zero: the columns [0, 12) of every row are read whatever N0 is, nothing
 * behind them; the finishing pn2_conv1x1_wgrad_cf writes the columns [0, N0) of the first layer's dW).  prev_red receives the first layer's two reductions as in
 * pn2_conv1x1_bwd.  _supported(): 1 for 96 x 64 and 64 x 64 with P % 64 == 0 from pn2_res_supported()'s row count on (options
 * SPLIT, SPLIT_RES, FUSE_FIRST on); PN2_EUNSUPPORTED otherwise (call pn2_conv1x1_bwd). */
int pn2_conv1x1_bwd_first_supported(int64_t P, int C_out, int C_in, int N0);
int pn2_conv1x1_bwd_first(const float *dZ, int ldz, const float *Y, int ldy, const float *coef, const float *W, int ldw,
                          const float *prev_Y, int ld_prev, const float *prev_affine, double *prev_red, float *dW, int lddw,
                          const float *X0, int ld0, int N0, void *cf_scratch, int64_t P, int C_out, int C_in,
                          const pn2_bn_coef_lazy *coef_lazy, pn2_stream_t stream);

/* Fused backward of one layer for the narrow, long layers (csrc/mlp_res.hip): dgrad AND wgrad in ONE pass over dZ / Y /
 * prev_Y -- autograd of model/pointnet_util.py:197,254,312 for conv + BatchNorm + ReLU.  dY is formed once per row
 * (as in pn2_conv1x1_dgrad), dXout = (dY W) masked by the previous layer's ReLU with its two BatchNorm-backward
 * reductions added to prev_red, dW (pitch lddw, caller zeroes) += dY^T relu(bn(prev_Y)).  prev_affine == NULL: the
 * layer input is prev_Y as stored, dXout = dY W unmasked, prev_red must be NULL.  The weight matrix stays in LDS for
 * the whole launch.  Only for shapes pn2_res_supported() accepts (C_out, C_in multiples of 32, <= 128); training-mode
 * BatchNorm only (no dbias).  pn2_conv1x1_fwd picks the matching weight-resident forward kernel by itself. */
int pn2_res_supported(int64_t P, int C_out, int C_in);
/* 1 if pn2_conv1x1_bwd runs (P, C_out, C_in) with this dZ form (Kpool = 0: dense) and input (masked: BatchNorm + ReLU of the
 * previous layer) in its fused kernel; 0: it would hand the layer to pn2_conv1x1_dgrad + pn2_conv1x1_wgrad. */
int pn2_bwd_res_supported(int64_t P, int C_out, int C_in, int Kpool, int masked);
int pn2_conv1x1_bwd(const float *dZ, int ldz, const float *dZp, int ldo, const int32_t *arg, int Kpool,
                    const float *Y, int ldy, const float *coef, const float *W, int ldw, const float *prev_Y,
                    int ld_prev, const float *prev_affine, float *dXout, int ldxo, double *prev_red, float *dW,
                    int lddw, int64_t P, int C_out, int C_in, const pn2_bn_coef_lazy *coef_lazy, pn2_stream_t stream);

/* Eval-mode fused module (csrc/eval.hip): rows -> L x (linear + ReLU) -> max over the neighbours in ONE launch, BatchNorm
 * folded into the weights by the caller (W' = diag(gamma / sqrt(var + eps)) W, b' likewise; rows of pitch ldw >=
 * round8(K), zero padded, 16-byte aligned).  model/pointnet_util.py:127-133 / :243-251 (gather, centre, concat) +
 * :194-199 / :251-256 / :309-312 (conv + BN + ReLU, max) under .eval() -- the reference's viewer loop pcdvis.py:118-136.
 * Input: X != NULL: plain rows [P, ldx] with P passed in `B` (FP modules, heads);  X == NULL: grouped rows formed on the
 * fly from idx [B,S,Knb] (xyz [B,N,3] minus new_xyz [B,S,3], cat with points [B,N,D]; xyz_first as pn2_group;
 * idx == NULL with S == 1, Knb == N, new_xyz == NULL: group_all, un-centred).  pool: 0 (out [P, ldo], ReLU applied) or
 * Knb (out [P / Knb, ldo]); Knb must be 16 or a multiple of 32.  L <= 4; activations of a 32-row tile stay in LDS: two
 * tiles of 32 x LP floats in 160 KiB, LP the least pitch = 4 mod 8 that holds round4(widest layer input) columns, i.e.
 * every K_l <= 636 (LP 636); wider chains are PN2_EINVAL.
 * Columns written: pool == 0, 16 and 32 write the columns [0, N_L) of their rows and nothing else.  pool > 32 first
 * zero-fills the WHOLE rows, (P / pool) * ldo floats (the target of the integer atomicMax), so there the columns
 * [N_L, ldo) end as 0.  Rows behind P (pool == 0) or P / pool are never touched.
 * NaN.  The hidden layers and the un-pooled store (pool == 0) apply ReLU as x < 0 ? 0 : x, which keeps a NaN like
 * torch.relu: a NaN in an input row makes that whole output row NaN and moves no other row.  Deviation from the reference,
 * pooled outputs only: the max over the neighbours is fmaxf followed by an integer atomicMax on the bits of the non-negative
 * result, both of which DROP a NaN (torch.max propagates it).  A diverged model therefore shows finite pooled features
 * here; the training-mode path (pn2_bn_relu_max) and the un-pooled outputs keep NaNs visible. */
typedef struct {
    const float *W;
    const float *bias;
    int K, N, ldw;
} pn2_eval_layer;
int pn2_fused_eval(const float *X, int ldx, const float *xyz, const float *points, const float *new_xyz,
                   const int64_t *idx, int B, int N, int S, int Knb, int D, int xyz_first,
                   const pn2_eval_layer *layers, int L, int pool, float *out, int ldo, pn2_stream_t stream);

/* ---- scatter-adds of the backward pass as segmented reductions (csrc/scatter.hip) ----------------------------
 * pn2_invert_index: idx [B, M] int64 with values in [0, T) -> members int32 [B, M], owners int32 [B, M]: the
 *   positions m of a cloud sorted by the value they point at (a counting sort per cloud; order inside one value is
 *   unspecified), and that value.  Out-of-range entries are dropped (their slots, at the end of the cloud's array,
 *   hold -1).  scratch: int32 [B, 2T+1]. */
int pn2_invert_index(const int64_t *idx, int B, int M, int T, int32_t *members, int32_t *owners, int32_t *scratch,
                     pn2_stream_t stream);
/* pn2_three_interp_bwd over the target-sorted 3-NN index (idx viewed as [B, 3N], T = S): runs of equal target are
 * summed in registers; a run that lies inside one chunk of the member list is STORED, the (at most two) runs that
 * straddle a chunk's ends are added atomically.  grad_points2 [B,S,D]: the caller MUST zero it (targets without
 * members are never written, and the straddling runs accumulate). */
int pn2_three_interp_bwd_seg(const float *grad_out, int ld, int col0, const int32_t *members, const int32_t *owners,
                             const float *weight, int B, int N, int S, int D, float *grad_points2, pn2_stream_t stream);
/* pn2_group_affine_bwd over the source-sorted ball-query index (idx viewed as [B, S*K], T = N).  G [B*N, ldg]:
 * the caller MUST zero it (same store-versus-atomic rule as pn2_three_interp_bwd_seg); dWx accumulated as in pn2_group_affine_bwd.  C <= 256.  dwx_scratch: float[PN2_DWX_REPLICAS * 3 *
 * round4(C)] zeroed by the caller, or NULL.  With it the per-workgroup dWx partials are added to one of
 * PN2_DWX_REPLICAS copies and a second small launch folds the copies into dWx (all resident workgroups finish
 * together; their 3*C same-word atomics on dWx itself cost up to 4x the rest of the launch). */
int pn2_group_affine_bwd_seg(const float *dZ, int ldz, const float *Y, int ldy, const float *coef, const float *xyz,
                             const float *new_xyz, const int32_t *members, const int32_t *owners, int B, int N, int S,
                             int K, int C, float *G, int ldg, float *dWx, int ldwx, float *dwx_scratch,
                             const pn2_bn_coef_lazy *coef_lazy, pn2_stream_t stream);

/* ---- the loss either side of the path ---------------------------------------
 * Replaces F.nll_loss(pred, target) of semseg.py:143 (weight == NULL; weight != NULL: its class-weighted form), reduction
 * "mean" (the criterion of pcdseg.py:178-179 is a cross entropy: pn2_cross_entropy_* below):
 *     loss = - sum_r w[t_r] * logp[r, t_r] / sum_r w[t_r]     over rows with t_r != ignore_index.
 * logp [R, ld >= C] log-probabilities, target int64[R].  A target outside [0, C) that is not ignore_index
 * turns the loss NaN (ATen raises a device assert).  workspace: pn2_nll_loss_workspace_bytes(R) bytes,
 * zeroed ONCE by the caller (the kernel leaves it reusable); do not share it between concurrent launches.
 * Outputs: *loss and *denom (= sum of the weights, kept for the backward).  The partial sums are fp64 and
 * combined in a fixed order: the result does not depend on scheduling. */
int64_t pn2_nll_loss_workspace_bytes(int64_t R);
int pn2_nll_loss_fwd(const float *logp, int ld, const int64_t *target, const float *weight, int64_t R, int C,
                     int64_t ignore_index, void *workspace, float *loss, float *denom, pn2_stream_t stream);
/* dlogp[r, c] = -(*grad_loss) * w[t_r] / (*denom) at c == t_r (and t_r != ignore_index), 0 elsewhere;
 * every element of dlogp [R, ld] is written. */
int pn2_nll_loss_bwd(const int64_t *target, const float *weight, int64_t R, int C, int64_t ignore_index,
                     const float *grad_loss, const float *denom, float *dlogp, int ld, pn2_stream_t stream);
/* pn2_cross_entropy_* (added within ABI 15: purely additive, no version change) replace the criterion of the SemanticKITTI loop,
 * pcdseg.py:178-179 `nn.CrossEntropyLoss()(logits.transpose(2, 1), target)`, with the semantics of
 * torch.nn.functional.cross_entropy(input, target, weight, ignore_index=, reduction=, label_smoothing=) for class-index targets:
 *     l_r = (1 - eps) * w[t_r] * (-log p[t_r]) + eps / C * sum_c w[c] * (-log p[c]),   p = softmax(x_r),   0 on ignored rows;
 *     reduction 0 "none": loss[r] = l_r;  1 "mean": *loss = sum_r l_r / sum_r w[t_r] (rows not ignored);  2 "sum": *loss = sum_r l_r.
 * x is read in place, C <= 64 classes, R rows, in one of two layouts:
 *     inner == 0: row-major, element (r, c) at x[r * ld + c], any pitch ld >= C (rows are read as float4 quads when ld % 4 == 0 and
 *                 x is 16-byte aligned, as dwords otherwise; nothing past column C of a row is touched);
 *     inner  > 0: class-strided [R / inner, C, inner], element (b, c, n) at x[b * C * inner + c * inner + n], row r = b * inner + n
 *                 (ld is ignored).
 * The transposed view of a contiguous [B, N, C] tensor that pcdseg.py passes IS the row-major case (ld = C).
 * weight: float[C] or NULL.  A target outside [0, C) that is not ignore_index never indexes weight or the row: the reduced loss
 * and that row's "none" entry turn NaN, and its gradient row is zero (the contract of pn2_nll_loss_*).
 * logsum: float[R], log sum_c exp(x[r, c] - max_c x[r, c]), kept for the backward (the row's log-sum-exp RELATIVE to its maximum:
 * max + log sum would round at the magnitude of the logits).  workspace (reductions 1, 2; NULL otherwise):
 * pn2_cross_entropy_workspace_bytes(R) bytes, zeroed ONCE by the caller; the kernel leaves it reusable; do not share it between
 * concurrent launches.  *denom = sum of the weights of the rows that count (reductions 1, 2).  fp64 partial sums combined in a
 * fixed order: the result does not depend on scheduling. */
int64_t pn2_cross_entropy_workspace_bytes(int64_t R);
int pn2_cross_entropy_fwd(const float *x, int ld, int64_t inner, const int64_t *target, const float *weight, int64_t R, int C,
                          int64_t ignore_index, double label_smoothing, int reduction, void *workspace, float *logsum, float *loss,
                          float *denom, pn2_stream_t stream);
/* One launch: dx[r, c] = g_r * [(1 - eps) * w[t_r] * (p_c - [c == t_r]) + eps / C * (p_c * sum_k w[k] - w[c])] in the layout of x
 * (same ld / inner), p_c recomputed from x and logsum.  g_r = *grad_out / *denom (mean), *grad_out (sum), grad_out[r] (none), all
 * read on the device.  Ignored rows and rows with an out-of-range target are written as zeros; bytes outside the C logical
 * columns of a padded row are never written. */
int pn2_cross_entropy_bwd(const float *x, int ld, int64_t inner, const int64_t *target, const float *weight, const float *logsum,
                          int64_t R, int C, int64_t ignore_index, double label_smoothing, int reduction, const float *grad_out,
                          const float *denom, float *dx, pn2_stream_t stream);
/* F.log_softmax(x, dim=-1) of the segmentation heads (model/pointnet2.py:175; :46, :103, :138) on rows whose C <= 64 logits
 * are the leading columns of a padded row (pitch ldx, a multiple of 4: the output of pn2_conv1x1_fwd as it stands -- no
 * slice copy): out[r, c] = x[r, c] - max_c x - log sum_c exp(x - max) for c < C, pitch ldo >= C. */
int pn2_log_softmax_fwd(const float *x, int ldx, int64_t R, int C, float *out, int ldo, pn2_stream_t stream);
/* Its backward, grad_x[r, c] = grad_out[r, c] - exp(out[r, c]) * sum_c grad_out[r, c], written at pitch ldgx <= 64 with
 * the pad columns c in [C, ldgx) set to zero: the padded gradient pn2_conv1x1_wgrad / _dgrad read as dZ. */
int pn2_log_softmax_bwd(const float *grad_out, int ldg, const float *out, int ldo, int64_t R, int C, float *grad_x, int ldgx,
                        pn2_stream_t stream);

/* ---- the optimiser step and the loader's per-cloud preparation --------------
 * pn2_adam_step replaces torch.optim.Adam(params, lr, betas=(0.9, 0.999), eps=1e-08, weight_decay) of
 * semseg.py:106-111 / pcdseg.py:133-138 (amsgrad off, L2 decay folded into the gradient) over ONE flat fp32 buffer
 * that all parameters alias; grad / exp_avg / exp_avg_sq are flat buffers of the same layout.  One launch:
 *     g += weight_decay * p;  m = lerp(m, g, 1 - beta1);  v = beta2 * v + (1 - beta2) * g * g;
 *     p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * `step` is t (>= 1) of this call.  step_dev != NULL: device int64[2] {steps taken so far, 0}; t = step_dev[0] + 1
 * is read on the device and step_dev[0] advanced by the launch itself (hipGraph replay needs no new arguments);
 * `step` is then ignored.  lr_dev != NULL: the learning rate is read from device memory instead of `lr`
 * (pcdseg.py:159-163 rewrites param_group['lr'] every epoch).  zero_grad != 0 also clears grad (the next
 * optimizer.zero_grad(), semseg.py:137) in the same pass. */
int pn2_adam_step(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, double lr, double beta1,
                  double beta2, double eps, double weight_decay, int64_t step, const float *lr_dev, int64_t *step_dev,
                  int zero_grad, pn2_stream_t stream);
/* pn2_sgd_step (added within ABI 15: purely additive, no version change) replaces torch.optim.SGD(params, lr, momentum,
 * dampening, weight_decay, nesterov, maximize=) -- the other branch of the reference's --optimizer switch (semseg.py:103-104,
 * partseg.py:113, clf.py:72, pcdseg.py:130-131: lr=0.01, momentum=0.9) -- with the conventions of pn2_adam_step: one launch over
 * one flat fp32 buffer, `step` = t (>= 1) of this call, step_dev = device int64[2] {steps taken, ticket} read and advanced by the
 * launch itself, lr_dev = the learning rate in device memory, zero_grad != 0 clears grad in the same pass.
 * The arithmetic is torch/optim/sgd.py::_single_tensor_sgd's, bit for bit: the scalars are doubles rounded to fp32 once
 * (wd = (float)weight_decay, om = (float)(1.0 - dampening), mu = (float)momentum, nl = (float)(-lr), or -(*lr_dev)), every
 * add(alpha=) is ONE rounding (fmaf), the mul_ of the buffer is rounded on its own:
 *     g = maximize ? -grad : grad;  if (weight_decay != 0) g = fmaf(wd, p, g);
 *     if (momentum != 0) { buf = t == 1 ? g : fmaf(om, g, buf * mu);  g = nesterov ? fmaf(mu, buf, g) : buf; }
 *     p = fmaf(nl, g, p)
 * (no dampening on the first step: torch clones the gradient into the new buffer).  momentum_buf is a flat twin of param, read
 * and written only when momentum != 0 (NULL, or ignored, otherwise: that path moves 12 B/element, 16 with zero_grad, against
 * 24 with a buffer and zero_grad).  float4 accesses where all pointers used are 16-byte aligned, a scalar kernel otherwise.
 * Returns PN2_EINVAL without a launch where torch.optim.SGD.__init__ raises (lr, momentum or weight_decay negative; nesterov
 * with momentum <= 0 or dampening != 0), for momentum != 0 without a buffer, and for n <= 0. */
int pn2_sgd_step(float *param, float *grad, float *momentum_buf, int64_t n, double lr, double momentum, double dampening,
                 double weight_decay, int nesterov, int maximize, int64_t step, const float *lr_dev, int64_t *step_dev,
                 int zero_grad, pn2_stream_t stream);
/* pn2_prepare_clouds replaces SemKITTI_Loader.__getitem__ (data_utils/SemKITTI_Loader.py:93-113) for a batch:
 * pcd_normalize (:23-30: x/70, y/70, z/3, (i-0.5)*2, clip to [-1,1]), pcd_jitter (:17-21: += noise) and
 * `pcd[choice]`, `label[choice]` (:110-113).
 *   raw        [rows, 4] fp32 x,y,z,intensity (the .bin row format, kitti_utils.py:200) of any number of scans kept
 *              resident in HBM; cloud b of the batch is rows [row_begin[b], row_begin[b] + row_count[b])
 *              (int64[B] each, device memory).
 *   raw_label  int32[rows] class per raw point, or NULL.
 *   noise      [*, 4] fp32 clipped jitter rows, one per RAW point (the reference jitters before it resamples, so
 *              duplicates share their noise); cloud b's rows start at noise_begin[b] (int64[B], device; NULL: the
 *              same rows as raw).  noise == NULL: no jitter (evaluation).
 *   choice     int64[B, N] row numbers inside each cloud (np.random.choice(M, N, replace=True)).
 * Outputs points [B, N, 4] fp32 and labels int64[B, N] (or NULL).  A choice outside [0, row_count[b]) sets
 * *bad_index (device int, caller zeroes, may be NULL) and reads row 0 (numpy raises IndexError). */
int pn2_prepare_clouds(const float *raw, const int64_t *row_begin, const int64_t *row_count, const int32_t *raw_label,
                       const float *noise, const int64_t *noise_begin, const int64_t *choice, int B, int N,
                       float *points, int64_t *labels, int *bad_index, pn2_stream_t stream);
/* pn2_prepare_shapes (added within ABI 15: purely additive, no version change) is the same gather for rows of any width: it
 * replaces PartNormalDataset.__getitem__ (data_utils/ShapeNetDataLoader.py:116-126: rotate_point_cloud, jitter_point_cloud,
 * `pointcloud[choice]`, `seg[choice]`, `normal[choice]`), the augmentation ModelNetDataLoader.__getitem__ intends
 * (ModelNetDataLoader.py:64-68) and S3DISDataLoader's jitter (S3DISDataLoader.py:71-75), for a batch.
 *   raw        [rows, C] fp32, 3 <= C <= 16, resident in HBM (4-byte alignment is all that is assumed: rows of 3, 6 or 9
 *              floats); cloud b is rows [row_begin[b], row_begin[b] + row_count[b]) (int64[B] each, device memory).
 *   raw_label  int32[rows] class per raw point, or NULL.
 *   rot        [B, 2] fp64 (cos, sin) of each cloud's angle about the up axis, or NULL.  Columns 0..2 become
 *              x' = f32(x*c + z*(-s)), y' = y, z' = f32(x*s + z*c) with the products and the sum in fp64, un-fused:
 *              np.dot(pc_f32, [[c,0,s],[0,1,0],[-s,0,c]]) stored into float32 (augmentation.py:36-44).  Other columns
 *              (the normals) are not rotated, as in the reference.
 *   noise      [*, noise_cols] fp64 clipped jitter rows (clip(0.01 * randn, -0.05, 0.05), augmentation.py:80), one per RAW
 *              point (duplicates share their jitter), cloud b's rows starting at noise_begin[b] (int64[B], device; NULL:
 *              the same rows as raw); 1 <= noise_cols <= C.  Columns < noise_cols become f32(noise + f64(value)), the
 *              value being the rotated fp32 one (augmentation.py:81, .astype(float32)); other columns are copied.
 *              noise == NULL: no jitter, noise_cols ignored.
 *   choice     int64[B, N] row numbers inside each cloud (np.random.choice(M, N, replace=True)); NULL: row n (needs
 *              row_count[b] >= N).
 * Outputs out [B, N, C] fp32 and labels int64[B, N] (or NULL).  A row number outside [0, row_count[b]) sets *bad_index
 * (device int, caller zeroes, may be NULL) and reads row 0.  Bad arguments return -1 without a launch. */
int pn2_prepare_shapes(const float *raw, int C, const int64_t *row_begin, const int64_t *row_count, const int32_t *raw_label,
                       const double *rot, const double *noise, int noise_cols, const int64_t *noise_begin,
                       const int64_t *choice, int B, int N, float *out, int64_t *labels, int *bad_index, pn2_stream_t stream);

/* ---- PointNet v1 (model/pointnet.py: STN3d / STNkd / PointNetEncoder / PointNetSeg), ABI 12 -----------------------------
 * Per-cloud transform, torch.bmm(x, trans) of PointNetEncoder.forward: out[b*N + n, j] = sum_i X[b*N + n, i] * T[b, i, j].
 * T [B, k, k] row-major (as torch holds `trans`), k <= 128; X / out position-major rows of pitch ldx / ldo (multiples of 4,
 * >= round4(k)); X's pad columns must be zero, out's pad columns [k, round4(k)) are written as zeros.  Any N. */
int pn2_point_transform(const float *X, int ldx, const float *T, int B, int N, int k, float *out, int ldo, pn2_stream_t stream);
/* Its backward: dX = dOut * T_b^T (dX != NULL, pitch lddx, pad columns written as zeros) and dT_b = sum_n X_n^T dOut_n
 * (dT != NULL: [B, k, k], STORED; X required).  dT is summed per 256-row slab into `workspace`
 * (pn2_point_transform_workspace_bytes(B, N, k) bytes, 4-byte aligned, contents irrelevant) and the slabs are added in a fixed
 * order by a second launch: run-to-run identical, no atomics.  dOut pitch ldd (multiple of 4, >= round4(k), pad columns zero).
 * Every argument is checked before the first launch: a refused call (PN2_EINVAL) has written neither dX nor dT. */
int64_t pn2_point_transform_workspace_bytes(int B, int N, int k);
int pn2_point_transform_bwd(const float *dOut, int ldd, const float *X, int ldx, const float *T, int B, int N, int k, float *dX, int lddx,
                            float *dT, void *workspace, pn2_stream_t stream);
/* pn2_bn_relu_max WITHOUT the ReLU (the encoder's bn3(conv3(x)) then torch.max over all points): out[g,c] = max_k bn(Y[g*K+k, c]),
 * bn(y) = fma(y - mean, scale, beta) from the affine block; arg[g,c] = the first k attaining it (a negative gamma selects the
 * smallest y; a zero gamma gives beta everywhere and names row 0).  Pitches as pn2_bn_relu_max; pad columns are written (0).
 * Any K.  Finite inputs only are tested: the comparison is a strict `>`, so a NaN is skipped, not propagated as torch.max does
 * (a group whose every bn(y) is NaN, or -inf, gives out = -inf and arg = 0). */
int pn2_bn_max(const float *Y, int ldy, const float *affine, int64_t G, int K, int C, float *out, int ldo, int32_t *arg,
               pn2_stream_t stream);
/* Its backward: dZp[g,c] = dOut[g,c] (pitch ldo like arg, pad lanes zero; dOut at any pitch ld_dout >= C), red (replicated,
 * caller zeroes) += sum_g dOut and sum_g dOut * yhat with yhat = (Y[g*K + arg[g,c], c] - mean) * invstd.  The pooled
 * pn2_conv1x1_dgrad / _wgrad (dZ == NULL, dZp / arg / Kpool = K) then serve the layer. */
int pn2_pool_bwd_reduce_noact(const float *dOut, int ld_dout, const int32_t *arg, int ldo, const float *Y, int ldy, const float *affine,
                              int64_t G, int K, int C, float *dZp, double *red, pn2_stream_t stream);
/* The broadcast-concat layer of PointNetSeg.conv1 (conv over cat([global.repeat(N), pointfeat])), factorised:
 *   Y[p, c] = (X W^T)[p, c] + bias[c] + gbias[p / rows_per_group, c]
 * with X the per-point columns (pointfeat), W their columns of the conv weight (pitch ldw: it may point into the full weight)
 * and gbias [P / rows_per_group, ldg] the per-cloud term W_g g_b.  pn2_conv1x1_fwd, then one pass that adds gbias and takes
 * the BatchNorm statistics (stats: replicated double[2*N] as pn2_conv1x1_fwd, caller zeroes; NULL: none). */
int pn2_conv1x1_fwd_gbias(const float *X, int ldx, const float *W, int ldw, const float *bias, const float *gbias, int ldg,
                          int64_t rows_per_group, float *Y, int ldy, int64_t P, int K, int N, double *stats, pn2_stream_t stream);
/* Its per-cloud gradient: s[g, c] = sum over the rows p of group g of dY[p, c], dY = c0*dZ + q1*(y - mean) + q0 (coef as from
 * pn2_bn_bwd_coef).  s [P / rows_per_group, lds] is STORED (pad columns up to min(lds, round4(C)) as zeros); per-slab sums
 * in `workspace` (pn2_group_colsum_workspace_bytes bytes) added in a fixed order: run-to-run identical. */
int64_t pn2_group_colsum_workspace_bytes(int64_t P, int64_t rows_per_group, int C);
int pn2_group_colsum(const float *dZ, int ldz, const float *Y, int ldy, const float *coef, int64_t P, int64_t rows_per_group, int C,
                     float *s, int lds, void *workspace, pn2_stream_t stream);

/* ---- PointNet v1 part segmentation (model/pointnet.py:153-228, PointNetDenseCls of partseg.py), ABI 13 -----------------------
 * convs1 (:178, :217-220) is a 1x1 conv over cat([expand, out1, out2, out3, out4, out5]) with 2064 per-cloud and 2880 per-point
 * columns.  The per-point part is ONE GEMM whose operand is the virtual concatenation of up to 8 sources, each read in place. */
typedef struct pn2_src {        /* one per-point source of a K-concatenated operand (host struct; the table is passed by pointer) */
    const float *X; int ldx;    /* [P, ldx] position-major rows, ldx % 4 == 0, ldx >= K */
    int K;                      /* its columns, K % 4 == 0 */
    const float *affine;        /* NULL: X as stored; else the affine block (float[4*K]) of the layer that produced X */
    int relu;                   /* with affine: 1 = relu(bn(x)), 0 = bn(x), both fmaf(x - mean, scale, beta) as pn2_bn_max */
} pn2_src;
/* Y[p,c] = sum_i act_i(X_i)[p,:] . W[c, k_i : k_i + K_i] + bias[c] + gbias[p / rows_per_group, c],  k_i = K_0 + .. + K_{i-1}.
 * W [N rows, pitch ldw >= sum K_i] may point into a wider weight at any column offset (one that is not a multiple of 4 floats
 * takes guarded scalar weight loads); gbias [P / rows_per_group, ldg] (ldg % 4 == 0, >= round4(N), 16-byte aligned) may be
 * NULL.  stats as pn2_conv1x1_fwd (replicated double[2*N], caller zeroes; NULL: none), taken on the final y in the same pass.
 * Y pitch ldy % 4 == 0, >= round4(N), pad columns written as 0.  1 <= nsrc <= 8, P < 2^31. */
int pn2_conv1x1_fwd_multi(const pn2_src *src, int nsrc, const float *W, int ldw, const float *bias, const float *gbias, int ldg,
                          int64_t rows_per_group, float *Y, int ldy, int64_t P, int N, double *stats, pn2_stream_t stream);
/* dW[m, k_i + j] += sum_p dY[p,m] act_i(X_i)[p,j] with dY = c0*dZ + q1*(y - mean) + q0 (coef of pn2_bn_bwd_coef), dense dZ, in ONE
 * launch over the virtual concatenation (fp32 atomics: dW is accumulated, the caller zeroes it).  dW pitch lddw >= sum K_i, any
 * column offset; dbias (may be NULL) += sum_p dY[p,m]. */
int pn2_conv1x1_wgrad_multi(const float *dZ, int ldz, const float *Y, int ldy, const float *coef, const pn2_src *src, int nsrc,
                            float *dW, int lddw, float *dbias, int64_t P, int M, pn2_stream_t stream);
/* dX_i = dY W[:, k_i : k_i + K_i] (k_i = K_0 + .. + K_{i-1}; unmasked, stored) into per-source outputs dX[i] of pitch lddx[i]
 * (% 4 == 0, >= K[i]; columns past K[i] are not written).  dX, lddx and K are host arrays of nsrc (1..8) entries.  One launch
 * of the pn2_conv1x1_dgrad core per source. */
int pn2_conv1x1_dgrad_multi(const float *dZ, int ldz, const float *Y, int ldy, const float *coef, const float *W, int ldw,
                            float *const *dX, const int *lddx, const int *K, int nsrc, int64_t P, int M, pn2_stream_t stream);
/* BatchNorm output without a ReLU consumed twice (out5 = bn5(conv5(.)) of :207-208, :219): densely (convs1) and by a max over
 * the K rows of each group (out_max, arg as from pn2_bn_max):
 *   dZ[g*K + k, c] = dDense[g*K + k, c] + (k == arg[g,c] ? dPool[g,c] : 0);  red (replicated, caller zeroes) += sum dZ, sum dZ * yhat,
 * yhat = (Y - mean) * invstd.  Every pitch % 4 == 0 and >= round4(C); pad columns of dZ written as 0.  dDense may alias dZ. */
int pn2_bn_bwd_reduce_noact_dense(const float *dDense, int ldd, const float *dPool, int ldp, const int32_t *arg, int lda,
                                  const float *Y, int ldy, const float *affine, int64_t G, int K, int C, float *dZ, int ldz,
                                  double *red, pn2_stream_t stream);

/* ---- Chamfer distance (model/chamfer.py), ABI 14 ---------------------------------------------------------------------------------
 * Nearest candidate of every query point: p1 [B,N,D] queries, p2 [B,M,D] candidates, 1 <= D <= 16 (larger: PN2_EUNSUPPORTED).
 *   d2(n,m) = fp32, DIFFERENCE form: t_k = p1[n,k] - p2[m,k]; d2 = t_0*t_0; d2 = fmaf(t_k, t_k, d2), k = 1 .. D-1 in order;
 *   idx[b,n] = the m of the smallest d2, the LOWEST m on equal d2;  dist[b,n] = sqrt(d2) (correctly rounded, once per query);
 *   sum (may be NULL) = (sum_b sum_n dist[b,n]) / B, added in a fixed order (fp64 partials per workgroup, then in index order).
 * dist, idx and sum are bit-identical from run to run; nothing of size N x M is written.  workspace:
 * pn2_chamfer_nn_workspace_bytes(B, N, M, D) bytes (host-only query, never 0 for a valid shape), 256-byte aligned, need not
 * be cleared.  B <= 65535, B*N < 2^31.
 * Non-finite coordinates (pinned by tests/test_chamfer_abi_gpu.py, observed on an MI355X): the search keeps a candidate only on
 * `d2 < best`, best starting at +inf, and a d2 that is NaN or +inf never passes it.  So a candidate with a NaN or infinite
 * coordinate is never chosen, and a query with one gets idx = 0 and dist = +inf, which makes sum +inf (torch.min would hand the
 * NaN on).  Such a row changes no other query's dist, idx or dp1 bits; in pn2_chamfer_bwd a non-finite query's dp1 row is NaN in
 * its non-finite components, and in dp2 it reaches candidate 0 of its own cloud only. */
int64_t pn2_chamfer_nn_workspace_bytes(int B, int N, int M, int D);
int pn2_chamfer_nn(const float *p1, const float *p2, int B, int N, int M, int D, float *dist, int64_t *idx, float *sum,
                   void *workspace, pn2_stream_t stream);
/* Backward of `sum` above for the upstream scalar *g (a DEVICE pointer: nothing is read back, the call can be captured):
 *   dp1[b,n,:] = (g / B) (p1[b,n,:] - p2[b,idx[b,n],:]) / dist[b,n], a zero row where dist == 0;
 *   dp2[b,idx[b,n],:] -= dp1[b,n,:] (fp32 atomics: the caller zeroes dp2; the order of the additions is not fixed).
 * Either output may be NULL. */
int pn2_chamfer_bwd(const float *p1, const float *p2, const float *dist, const int64_t *idx, const float *g, int B, int N, int M,
                    int D, float *dp1, float *dp2, pn2_stream_t stream);

/* ---- Segmentation metrics (pcd_utils.py:65-210, pcdseg.py:58-97), added within ABI 15 (purely additive: no version change) ----------
 * Confusion table of B clouds of N rows: logp holds B*N rows of pitch ld >= C whose first C columns are the classes (columns
 * c >= C -- the pad of a [B*N, round4(C)] buffer -- may hold anything, NaN included: they never influence the result), target
 * B*N labels.  pred(row) = the index of the row's largest entry, the LOWEST index on equal values; a NaN counts as largest and the
 * first NaN wins; a row of all -inf predicts 0 (what torch.max(dim)[1] and argmax return).  Cloud b's table is int64 [C + 1, C] at
 * conf + b * conf_stride: a row with target t in [0, C) adds 1 at [t, pred], any other target adds 1 at [C, pred] (such a point
 * joins no class's target set but still counts in the union of the class it was predicted as); rows whose target equals
 * ignore_index are skipped (INT64_MIN: none).  The call ADDS into conf (the caller zeroes it) with 64-bit integer atomics: the
 * result does not depend on scheduling.  conf_stride = 0 pools the batch into one table, (C + 1) * C gives one table per cloud.
 * pred (may be NULL) receives the B*N predictions.  1 <= C <= 64 (larger: PN2_EUNSUPPORTED, nothing launched); B*N == 0 is a
 * no-op returning 0.  Rows are read as float4 quads when ld % 4 == 0 and logp is 16-byte aligned, one float at a time otherwise. */
int pn2_seg_confusion(const float *logp, int ld, const int64_t *target, int B, int64_t N, int C, int64_t ignore_index, int64_t *conf,
                      int64_t conf_stride, int64_t *pred, pn2_stream_t stream);

/* ---- The KITTI demo's frame path (pcdvis.py:115-144), added within ABI 15 (purely additive: no version change) ------------------------
 * Small tables below (group table, calibration, disc rows) are HOST arrays: they are checked on the host and travel inside the
 * launch.  Everything else is device memory.  No entry point allocates or waits: each call can be captured in a graph.
 *
 * pn2_seg_predict replaces `logits[0].argmax(-1)` (pcdvis.py:136) and the class merges of KITTI_2_Common.__call__ /
 * SemKITTI_2_Common.__call__ (data_utils/kitti_utils.py:41-58, :92-117).  logp: R rows of pitch ld >= C, the first C columns are
 * the classes (1 <= C <= 64; larger: PN2_EUNSUPPORTED).  G == 0: pred[r] = the row's arg-max exactly as pn2_seg_confusion defines
 * it (lowest index on ties, the first NaN wins, an all -inf row gives 0).  G > 0 (<= 64): group g consists of the classes
 * member[group_begin[g] .. group_begin[g + 1]) (host int32; every group non-empty, members in [0, C), at most 256 members in
 * all); merged[r, g] (pitch ldm >= G) = the largest of its members, NaN if any member is NaN (Tensor.max(dim)), and pred[r] = the
 * arg-max over the G group values by the same rule.  pred and merged may each be NULL (merged needs G > 0). */
int pn2_seg_predict(const float *logp, int ld, int64_t R, int C, const int32_t *group_begin, const int32_t *member, int G,
                    int64_t *pred, float *merged, int ldm, pn2_stream_t stream);
/* pn2_project_points replaces Semantic_KITTI_Utils.project_3d_to_2d (kitti_utils.py:313-336) with numpy's own arithmetic.  xyz: N
 * rows of pitch ldx >= 3 floats (the first three columns of [N, 4] scans are read in place); RT host double[12] (3 x 4, row-major:
 * [R | T]), P host double[9] (3 x 3).  Per point, every operation rounded separately (no fused multiply-add):
 *   c_k = f32(((RT[k][0]*x + RT[k][1]*y) + RT[k][2]*z) + RT[k][3]*1.0)   in fp64 on the fp32 inputs,
 *   q_k = f32((P[k][0]*c_0 + P[k][1]*c_1) + P[k][2]*c_2)                 in fp64 on the rounded fp32 c,
 *   pts_2d[n] = (q_0 / q_2, q_1 / q_2)                                   IEEE fp32 divisions (inf / NaN at the camera plane).
 * pix (int32 [N, 2], may be NULL; so may pts_2d, not both) = the truncation toward zero that `.astype(np.int32)` performs
 * (kitti_utils.py:374); a point with a component that is not finite or whose magnitude is >= 2^31 gets INT32_MIN in BOTH (numpy's
 * cast is undefined there) and is skipped by pn2_splat_discs.
 * RT == NULL and P == NULL (pts_2d == NULL): the top view's centres instead (kitti_utils.py:387-390), in Python's arithmetic:
 * X = trunc(-x*800 + 600), Y = trunc(-y*800 + 400) in fp64, pix[n] = (Y, X) as :390 passes them; INT32_MIN in both when either
 * is not finite or >= 2^31 in magnitude (Python's int() raises there). */
int pn2_project_points(const float *xyz, int ldx, int64_t N, const double *RT, const double *P, float *pts_2d, int32_t *pix,
                       pn2_stream_t stream);
/* pn2_splat_discs + pn2_splat_resolve replace the drawing loops of draw_2d_points / draw_2d_top_view (kitti_utils.py:368-392:
 * `cv2.circle(image, (x, y), r, c, -1)` per point, so a pixel shows the LAST point that covered it).
 * pn2_splat_discs clears owner (uint32 [H * W]; the clear is part of the call) and sets owner[y * W + x] = max(i + 1) over the
 * points i whose disc covers pixel (x, y): integer maxima, the result does not depend on scheduling.  pix int32 [N, 2] centres
 * (x = column, y = row); a centre with INT32_MIN in either component is skipped; discs are clipped to the image.  The disc is
 * the host table half_width[2 * radius + 1]: its row dy = j - radius covers dx in [-half_width[j], half_width[j]] (-1: nothing).
 * radius <= 32 (larger: PN2_EUNSUPPORTED), H * W < 2^31, N < 2^31. */
int pn2_splat_discs(const int32_t *pix, int64_t N, const int32_t *half_width, int radius, int H, int W, uint32_t *owner,
                    pn2_stream_t stream);
/* out (uint8 [H, W, 3]) = colors[label[owner - 1]] where a pixel has an owner, else background (uint8 [H, W, 3]; NULL: zeros).
 * colors uint8 [C, 3], label int64 [N].  A label outside [0, C) leaves the background and sets *err (device int, caller zeroes,
 * may be NULL) to 1, as pn2_gather_rows does (the reference's `colors[pred]` raises IndexError). */
int pn2_splat_resolve(const uint32_t *owner, int H, int W, const int64_t *label, int64_t N, const uint8_t *colors, int C,
                      const uint8_t *background, uint8_t *out, int *err, pn2_stream_t stream);
/* pn2_depth_splat + pn2_depth_resolve (+ pn2_splat_resolve for the colours) replace the demo's 3-D ego view, Window_Manager.update
 * (pcdvis.py:31-51, called at :143): the cloud seen through a fixed pinhole camera (config/ego_view.json), drawn as square points
 * of integer size (config/render_option.json) with a depth test.  THE RASTERISATION RULE IS STATED HERE, NOT TAKEN FROM open3d,
 * against which it could not be checked.  xyz: N rows of pitch ldx >= 3 floats, read in place; extrinsic host double[12] (3 x 4,
 * row-major: [R | t], world -> camera, +X right, +Y down, +Z forward); intrinsic host double[4]: fx, fy, cx, cy.  Per point i, in
 * fp64 on the fp32 coordinates, every product and sum rounded separately in this order (no fused multiply-add):
 *   c_k = ((E[k][0]*x + E[k][1]*y) + E[k][2]*z) + E[k][3],  Z = c_2;  drawn iff z_near < Z && Z < z_far (a NaN Z is not);
 *   d = f32(Z);  xw = ((fx*c_0)/Z + cx) + 0.5,  yw = ((fy*c_1)/Z + cy) + 0.5  (the principal point counts pixel centres);
 *   skipped if xw or yw is not finite or reaches 2^30 in magnitude (compared as doubles, before any integer conversion);
 *   OpenGL's non-antialiased point of size s: columns x0 .. x0 + s - 1 with x0 = floor(xw + (s even ? 0.5 : 0.0)) - s / 2,
 *   rows likewise from yw (row = y, top row first), clipped to [0, W) x [0, H).
 * Every covered pixel takes the minimum of key = bits(d) << 32 | i (64-bit unsigned; zkey [H * W], set to all-ones by the call
 * itself): the nearest point wins, the lowest index among equal float32 depths (GL_LESS in draw order); integer minima commute,
 * the result does not depend on scheduling.  0 < z_near < z_far <= 3e38, so d is finite and its bits order like its value.
 * 1 <= point_size <= 16 (else PN2_EUNSUPPORTED), H * W < 2^31, N < 2^31; N == 0 leaves the empty image. */
int pn2_depth_splat(const float *xyz, int ldx, int64_t N, const double *extrinsic, const double *intrinsic, double z_near,
                    double z_far, int point_size, int H, int W, uint64_t *zkey, pn2_stream_t stream);
/* owner (uint32 [H * W], may be NULL) = the visible point's index + 1, 0 where the pixel is empty: the format pn2_splat_resolve
 * colours from.  depth (float [H * W], may be NULL) = that point's float32 depth, +inf where empty. */
int pn2_depth_resolve(const uint64_t *zkey, int H, int W, uint32_t *owner, float *depth, pn2_stream_t stream);
/* pn2_scan_filter (added within ABI 15: purely additive, no version change) replaces Semantic_KITTI_Utils.get
 * (data_utils/kitti_utils.py:183-227: the class map :204-213, the drop of class 0 and the shift :215-219, the `inview` subset
 * :221-225) with points_basic_filter (:259-280: hv_in_range :237-249, box_in_range :251-257) and the boolean-index compaction,
 * for a batch of B raw scans that lie back to back in device memory.  Three plain launches on the caller's stream; no host
 * synchronisation, no allocation, no workgroup waits on another, no atomic decides a position.
 *   raw        [rows, 4] fp32, the .bin rows (16-byte aligned); scan b is rows [row_begin[b], row_begin[b] + row_count[b])
 *              (int64[B] each, DEVICE memory: the convention of pn2_prepare_clouds).
 *   raw_label  uint32[rows], the .label words, or NULL: an unlabelled scan, no class map and no class drop.
 *   max_rows   host upper bound of every row_count[b], 0 <= max_rows < 2^31; it sizes the grid and the workspace only.  Tiles of
 *              PN2_SCAN_TILE rows that start at or beyond the device-side row_count[b] do nothing, so a captured launch stays
 *              valid when the count changes.  A negative row_count counts as 0.
 *   lut        int32[lut_len] (device): raw class -> training class, -1 = not in the map (unused when raw_label is NULL).
 *   fov        host float[4] t0, t1, t2, t3, or NULL: no angular test (subset 'all').
 *   box        host float[8]: lower, upper bound of x, y, z, d; or NULL: no box test (what `get` does for subset 'all').
 *   out_begin  int64[B] (device): where scan b's kept rows start in the outputs; may equal row_begin.  Outputs must not alias
 *              inputs, and every output must hold out_begin[b] + (the kept count of scan b) rows for every b.
 * THE RULE, per row (x, y, z, intensity) with label word w:
 *   sem = w & 0xFFFF;  c = sem < lut_len ? lut[sem] : -1;  kept only if c > 0; the output class is c - 1.  (c < 0: the reference
 *   raises KeyError; here the row is dropped and PN2_SCAN_ERR_CLASS is set.)
 *   d = sqrtf((x*x + y*y) + z*z): fp32, every operation rounded on its own (no fused multiply-add), correctly rounded square
 *   root -- numpy's np.sqrt(x**2 + y**2 + z**2).
 *   box: x > box[0] && x < box[1] && y > box[2] && y < box[3] && z > box[4] && z < box[5] && d > box[6] && d < box[7], strict
 *   float32 comparisons (:251-257); a NaN or infinite coordinate fails them.
 *   angles: az = (float)atan2((double)y, (double)x), el = (float)atan2((double)z, (double)d); kept iff t0 < az && az < t1 &&
 *   t2 < el && el < t3, strict, in float32.  The fp64 atan2 rounded to float32 is deliberate: numpy's float32 arctan2 is not
 *   correctly rounded and differs between builds.  IEEE special cases hold: atan2(+0, -0) = pi, atan2(+-0, +0) = +-0; the point
 *   (0, 0, 0) has az = el = 0 and is kept, as in the reference.
 *   compaction is STABLE: kept rows keep their scan order, so the output is the reference's points[mask], identical from run
 *   to run.
 * Outputs: out_points fp32 [., 4] (16-byte aligned; the kept rows, bit for bit); out_labels int32 (c - 1; 0 for an unlabelled
 * scan; may be NULL); out_index int32 (the raw row inside its scan each kept row came from, strictly increasing; may be NULL);
 * out_count int64[B]; err (device int, caller zeroes, may be NULL) receives
 *   PN2_SCAN_ERR_CLASS  a raw class outside the map (sem >= lut_len or lut[sem] < 0): the row is dropped;
 *   PN2_SCAN_ERR_ROWS   a row_count[b] above max_rows: the rows beyond max_rows are ignored.
 * workspace: pn2_scan_filter_workspace_bytes(B, max_rows) bytes of device memory, 16-byte aligned (a one-byte flag per row of
 * every tile, a count and an offset per tile); its content need not be kept between calls.  PN2_EINVAL without a launch for a null
 * required pointer, B < 1 or B > 65535, max_rows < 0 or >= 2^31, lut_len < 1 (or a null lut) with labels given, a misaligned
 * raw / out_points / workspace; pn2_scan_filter_workspace_bytes returns PN2_EINVAL for such B / max_rows. */
#define PN2_SCAN_TILE 1024
#define PN2_SCAN_ERR_CLASS 1
#define PN2_SCAN_ERR_ROWS 2
int64_t pn2_scan_filter_workspace_bytes(int B, int64_t max_rows);
int pn2_scan_filter(const float *raw, const uint32_t *raw_label, const int64_t *row_begin, const int64_t *row_count, int B,
                    int64_t max_rows, const int32_t *lut, int lut_len, const float *fov, const float *box, const int64_t *out_begin,
                    float *out_points, int32_t *out_labels, int32_t *out_index, int64_t *out_count, int *err, void *workspace,
                    pn2_stream_t stream);

/* ---- k nearest neighbours and the vote over them (csrc/knn.hip), added within ABI 15 (purely additive: no version change) ----------
 * K nearest candidates of every query.  query [B,N,3], cand [B,M,3], 1 <= K <= 32, K <= M.
 * d2 = pair_dist of geometry.hip (expanded form, the arithmetic of pn2_three_nn and pn2_square_distance, bit for bit).
 * idx [B,N,K] int64, dist [B,N,K] float32 (may be NULL): ascending d2, equal d2 in ascending candidate index
 * (= the first K of a stable sort of the row of distances).  A candidate whose d2 is NaN or +inf is never selected;
 * slots left unfilled hold idx = M and dist = +inf (as pn2_ball_query writes N for an empty ball).
 * n_query / n_cand (device int64 [B], either may be NULL = N / M): only the first n_query[b] queries are written and only
 * the first n_cand[b] candidates searched (clamped to [0,N] / [0,M]); rows at and beyond n_query[b] are left untouched.
 * K > 32: PN2_EUNSUPPORTED, nothing launched.  K < 1, K > M, null pointers, non-positive sizes: PN2_EINVAL.
 * (B <= 65535, N <= 2^31 - 256: PN2_EINVAL beyond.) */
int pn2_knn(const float *query, const float *cand, int B, int N, int M, int K, const int64_t *n_query, const int64_t *n_cand,
            int64_t *idx, float *dist, pn2_stream_t stream);
/* Majority label of each row's neighbours.  idx/dist [B,N,K] as pn2_knn wrote them, cand_label int64 [B,M].
 * Slot k of a row VOTES iff 0 <= idx[k] < M and !(dist[k] > max_d2)   (max_d2 = +inf: no cut-off).
 * Winner = the label with the most voting slots; among labels with equally many, the one whose first voting slot comes
 * first (i.e. whose nearest voter is nearest).  No voting slot: the row's result is `fill`.
 * lut (int32 [L], may be NULL): the result is lut[label]; a winning label outside [0,L) gives `fill` and sets *err |= 1.
 * Without a lut the result is the label's low 32 bits.
 * dst (int32 [B,N], may be NULL): row n of cloud b is written at out[b*out_stride + dst[b,n]] instead of out[b*out_stride + n];
 * a dst outside [0,out_stride) is skipped and sets *err |= 2.  Only the first n_query[b] rows are processed (NULL = N).
 * out int32.  err: device int32, may be NULL.  1 <= K <= 32 (larger: PN2_EUNSUPPORTED, nothing launched).
 * Every candidate slot votes once: a candidate that appears several times among the M (a cloud drawn with replacement) votes
 * once per appearance.  Integer arithmetic only: out is exact and the same from run to run.
 * PN2_EINVAL: null idx / dist / cand_label / out, non-positive sizes, K < 1, out_stride < 1, out_stride < N without a dst,
 * a lut with L < 1. */
int pn2_knn_vote(const int64_t *idx, const float *dist, const int64_t *cand_label, int B, int N, int M, int K, float max_d2,
                 const int64_t *n_query, int32_t fill, const int32_t *lut, int L, const int32_t *dst, int64_t out_stride,
                 int32_t *out, int32_t *err, pn2_stream_t stream);

/* ---- local PCA: surface normals and covariance eigenvalues over neighbour lists (csrc/normals.hip), added within ABI 15 (purely
 * additive: no version change) ----------
 * For every row of idx: the covariance of the row's neighbourhood, its three eigenvalues and the unit eigenvector of the
 * smallest (the surface normal).  One plain launch on the caller's stream; no allocation, no host synchronisation, no atomics
 * except the OR into err; no output depends on the order in which lanes run, so the bytes are the same from run to run.
 *   cand [B,M,ldc], query [B,N,ldq] fp32, 3 <= ld <= 16, columns 0..2 = x, y, z (a [., 4] scan is read where it lies).  query is
 *        read only for the sign and may be NULL when viewpoint is NULL; a self-search passes the same pointer twice.
 *   idx  [B,N,K] int64 as pn2_knn (or pn2_ball_query) writes it, any K >= 1.   dist [B,N,K] fp32, may be NULL (no cut-off).
 *   n_query  device int64 [B] or NULL, pn2_knn's meaning: rows at and beyond the count are left untouched in every output.
 *   viewpoint  device fp32 [B,3] or NULL.
 *   normal [B,N,ldn] (ldn >= 3; ONLY columns 0..2 of each row are written: the pointer may be offset into a wider row),
 *   eig fp32 [B,N,3], cov fp64 [B,N,6], count int32 [B,N]: each may be NULL.  err: device int32, caller zeroes, may be NULL.
 * VALID SLOTS.  Slot k of a row is valid iff 0 <= idx[k] < M and !(dist[k] > max_d2) -- pn2_knn_vote's predicate: pn2_knn's
 *   empty slots (idx = M) drop out.  n = the number of valid slots.  A candidate that appears several times counts once per
 *   appearance (pn2_ball_query pads by repetition: those are its weights, as in the vote).
 * COVARIANCE, IEEE fp64, one pass in ascending slot order, nothing fused.  p0 = the first valid slot's point;
 *   d = double(p) - double(p0) (exact);  S1 += d;  S2_ab += d_a * d_b for the six a <= b;  m = S1 / n;
 *   C_ab = S2_ab / n - m_a * m_b   (divisor n, not n - 1).   cov = xx, xy, xz, yy, yz, zz of C, bit for bit this statement.
 *   (The shift by a member of the neighbourhood is what makes one pass safe: |d| is of the size of the neighbourhood.)
 * EIGEN-SOLVE, fp64: l0 <= l1 <= l2 the eigenvalues of C, a computed value below zero written as +0.0; eig = the three rounded
 *   to fp32; u = a unit eigenvector of l0.  Cyclic Jacobi, a fixed number of sweeps (csrc/sym_eig3.h): a C that is already
 *   diagonal is not rotated, u is then the axis of its smallest entry, the lowest axis among equal entries.
 * SIGN.  With a viewpoint v: s = (u_x w_x + u_y w_y) + u_z w_z in fp64, w = double(v) - double(q), q the row's query point;
 *   u is flipped iff s < 0.  Without a viewpoint, or when s == 0: flipped iff u_z < 0; if u_z == 0, iff u_y < 0; if that is 0 too,
 *   iff u_x < 0 (align with +z, then +y, then +x).  normal = the signed u rounded to fp32.
 * DEGENERATE ROWS.  n < 3: normal = three +0.0, eig and cov what the rule gives (all +0.0 for n = 0), count = n,
 *   *err |= PN2_PCA_ERR_FEW.  A valid slot's point not finite, or the query's while a viewpoint is in use: normal and eig are
 *   the quiet NaN 0x7FC00000, cov 0x7FF8000000000000, count = n, *err |= PN2_PCA_ERR_NONFINITE (and not PN2_PCA_ERR_FEW).
 * PN2_EINVAL, nothing launched and every output untouched: a null cand or idx, a viewpoint without a query, non-positive sizes,
 * a pitch out of range (ldc, ldq of a given query outside [3,16], ldn < 3 with a normal), B > 65535, N > 2^31 - 256. */
#define PN2_PCA_ERR_FEW 1
#define PN2_PCA_ERR_NONFINITE 2
int pn2_local_pca(const float *query, int ldq, const float *cand, int ldc, const int64_t *idx, const float *dist, int B, int N, int M,
                  int K, float max_d2, const int64_t *n_query, const float *viewpoint, float *normal, int ldn, float *eig, double *cov,
                  int32_t *count, int32_t *err, pn2_stream_t stream);

/* ---- grid kNN: k nearest within a radius on a uniform grid (csrc/grid_knn.hip), added within ABI 15 (purely additive: no version
 * change) ----------
 * pn2_grid_build bins the candidates of B clouds by cell once; pn2_grid_knn lets every query look at the 27 cells around its own.
 * Plain launches on the caller's stream (six for the build, one for a search); no allocation, no host synchronisation, no thread
 * waits for another thread's write, no float atomics.  THE RESULT IS DEFINED BY THE GRID, not as "equal to brute force"; when
 * cell[a] >= sqrt((double)max_d2) * (1 + 2^-20) on every axis it EQUALS the brute-force "K nearest with d2 <= max_d2" in the same
 * arithmetic ("Grid kNN", has the derivation).
 *   cand [B,M,ldc], query [B,N,ldq] fp32, 3 <= ld <= 16, columns 0..2 = x, y, z (a [., 4] scan is read where it lies): pn2_knn's dense
 *        layout, so idx / dist feed pn2_knn_vote and pn2_local_pca unchanged.
 *   n_cand / n_query  device int64 [B] or NULL (= M / N), clamped to [0,M] / [0,N]: only the first n_cand[b] candidates are indexed;
 *        rows at and beyond n_query[b] are left untouched in every output.
 *   origin, cell   HOST double[3] each: cell[a] finite and > 0, origin[a] finite (pn2_voxel_grid's check).
 * CELL.  pn2_voxel_grid's rule, shared (csrc/voxel_cell.h): per axis q_a = floor(((double)p_a - origin[a]) / cell[a]), IEEE fp64, each
 *   operation rounded on its own; a row is VALID iff -2^20 <= q_a < 2^20 on all three axes (NaN and +-inf fail); the key is the same
 *   63-bit word.
 * INVALID ROWS.  An invalid CANDIDATE is not indexed and never returned; it sets PN2_GRID_ERR_CAND (in pn2_grid_build's err).  An
 *   invalid QUERY gets every slot empty and count = 0; it sets PN2_GRID_ERR_QUERY (in pn2_grid_knn's err).
 * CANDIDATE SET of a query: the indexed candidates of its own cloud whose cell differs from the query's by d in {-1,0,1}^3 -- 27
 *   cells, the centre included.  A neighbour cell outside [-2^20, 2^20) on any axis does not exist (checked per axis BEFORE the
 *   key is formed).  Clouds never share cells, even at equal coordinates.
 * DISTANCE.  Difference form in fp32, pn2_chamfer_nn's arithmetic at D = 3 bit for bit: t_a = q_a - p_a; d2 = t_x * t_x;
 *   d2 = fmaf(t_y, t_y, d2); d2 = fmaf(t_z, t_z, d2).  (Deliberately not pn2_knn's expanded form: at scan scale that carries about
 *   5e-4 m^2 of cancellation error, comparable with a small cut-off.)
 * SELECTION.  The candidates of the set with d2 <= max_d2 take part (a NaN d2 fails; max_d2 = +inf is allowed: "the K nearest of the
 *   27 cells").  The result is the first K of them in ascending (d2, candidate index) order, the compare lexicographic on the PAIR:
 *   it does not depend on the order in which candidates are met.  Empty slots hold idx = M, dist = +inf as pn2_knn writes them.  A
 *   candidate that appears several times among the M is several candidates.  There is no K <= M requirement: short rows pad.
 *   idx int64 [B,N,K];  dist fp32 [B,N,K] or NULL;  count int32 [B,N] or NULL: the number of candidates that took part, NOT capped
 *   by K (the ball's population: count > K says K truncated).  err: device int32, caller zeroes, may be NULL.
 * SELF-SEARCH.  query == NULL (then N must equal M, ldq and n_query are ignored): the queries are the candidates themselves, the
 *   coordinates the build copied; every row below the candidate count THE BUILD READ is written (an indexed row finds itself at
 *   d2 = 0, an invalid row as above).  flags = PN2_GRID_VISIT_SORTED: lane i serves the i-th RECORD of the cell-sorted copy and
 *   writes at that record's row, so neighbouring lanes walk the same cells; without it, and always with a query, lane i serves
 *   row i.  The outputs are byte-identical either way.
 * WORKSPACE.  pn2_grid_workspace_bytes(B, M) bytes of device memory, 16-byte aligned.  UNLIKE THE OTHER WORKSPACES OF THIS LIBRARY IT
 *   PERSISTS: it may hold anything before pn2_grid_build, which fills it, and every pn2_grid_knn that uses it reads it (and
 *   writes nothing to it), with the same B, M, origin and cell as the build.  One build serves any number of searches.  Per cloud:
 *   a table of the power of two >= 2 * M slots of 16 bytes, a 16-byte record and a 4-byte word per row.
 * Everything is the same from run to run, byte for byte: which slot a cell lands in and the order of the records inside a cell
 * differ, but populations and starts are integer sums and the selection compares pairs.
 * 1 <= K <= 32; K > 32: PN2_EUNSUPPORTED, nothing launched.  PN2_EINVAL, nothing launched and nothing written: a null cand / origin /
 * cell / workspace / idx, B < 1 or B > 65535, M < 1 or M > PN2_VOXEL_MAX_ROWS, N < 1 or N > 2^31 - 256, K < 1, a pitch outside 3..16,
 * a self-search with N != M, unknown flags, cand / query not 4-byte or workspace not 16-byte aligned, a bad grid;
 * pn2_grid_workspace_bytes returns PN2_EINVAL for such B / M. */
#define PN2_GRID_ERR_CAND 1
#define PN2_GRID_ERR_QUERY 2
#define PN2_GRID_VISIT_SORTED 1          /* flags of pn2_grid_knn */
int64_t pn2_grid_workspace_bytes(int B, int64_t M);
int pn2_grid_build(const float *cand, int ldc, int B, int M, const int64_t *n_cand, const double *origin, const double *cell,
                   int32_t *err, void *workspace, pn2_stream_t stream);
int pn2_grid_knn(const float *query, int ldq, int B, int N, int M, int K, float max_d2, const int64_t *n_query,
                 const double *origin, const double *cell, const void *workspace, int flags,
                 int64_t *idx, float *dist, int32_t *count, int32_t *err, pn2_stream_t stream);

/* ---- ICP step: rigid scan registration on the grid index (csrc/icp.hip), added within ABI 15 (purely additive: no version
 * change) ----------
 * pn2_icp_step does ONE Gauss-Newton iteration of point-to-plane or point-to-point ICP for B source clouds, each against its own
 * target cloud, which pn2_grid_build has binned.  Two plain launches on the caller's stream; no allocation, no host
 * synchronisation, no float atomics, no thread waits for another thread's write.  tests/icp_ref.py restates the rule in numpy.
 *   src [B,N,lds], tgt [B,M,ldt] fp32, 3 <= ld <= 16, columns 0..2 = x, y, z.   n_src  device int64 [B] or NULL (= N), clamped to [0,N].
 *   tgt_normal [B,M,ldn] fp32, 3 <= ldn <= 16, only columns 0..2 are read (it may point into [.,6] rows); NULL for PN2_ICP_POINT.
 *   origin, cell, grid_workspace: what pn2_grid_build was given and filled for tgt, with the same B, M.  max_d2: pn2_grid_knn's.
 *   T  device fp64 [B,12], rows of [R | t] (3 x 4, row-major), read and written.   sums fp64 [B,28].   count int64 [B].
 *   x fp64 [B,6].   status, iters int32 [B], read and written.   corr int64 [B,N] or NULL.   err int32, caller zeroes, or NULL.
 *   workspace: pn2_icp_workspace_bytes(B, N) bytes of device memory, 8-byte aligned; it may hold anything.
 * FROZEN CLOUDS.  A cloud whose status has PN2_ICP_CONVERGED or PN2_ICP_SINGULAR set on entry is frozen: none of its outputs is
 *   touched and its rows are not walked.  PN2_ICP_EVAL_ONLY ignores the freeze (and does not read status).
 * PER ROW i < n_src[b] of the other clouds, IEEE fp64, each operation rounded on its own, nothing fused:
 *   s = double(src[i,0..2]);  p_a = ((R_a0 s_0 + R_a1 s_1) + R_a2 s_2) + t_a;  p32 = float(p).
 *   j = pn2_grid_knn's K = 1 answer for the query p32 with this max_d2: the 27 cells, the fp32 difference-form distance, the
 *   smallest (d2, index).  No candidate: the row takes no part, corr = M.  p32 not finite or outside the grid: the row takes no
 *   part, corr = M, *err |= PN2_ICP_ERR_QUERY.  Otherwise corr = j,  q = double(tgt[j]),  e = p - q  (from p, not from p32).
 *   PLANE: n = double(tgt_normal[j]); n not finite or three zeros (PN2_PCA_ERR_FEW's normal): the row takes no part (corr = j).
 *     r = (n_x e_x + n_y e_y) + n_z e_z;   J = (c, n) with c_x = p_y n_z - p_z n_y, c_y = p_z n_x - p_x n_z, c_z = p_x n_y - p_y n_x.
 *     The row's 28 terms: J_k J_l for the 21 pairs k <= l (row-major), J_k r (6), r r.
 *   POINT: the same three times with n = (1,0,0), (0,1,0), (0,0,1), evaluated as written: 84 terms a row.
 *   count = the rows that took part (rows, not residuals).
 * SUMS.  sums[b] = the 28 fp64 sums of these terms: A's upper triangle row-major, b, E.  The order of summation is a function of
 *   (B, N) alone and is not stated otherwise; it does not depend on how lanes are scheduled: the same bytes from run to run.
 * SOLVE (not with PN2_ICP_EVAL_ONLY).  A x = -b by fp64 Cholesky in index order.  The cloud is SINGULAR if count < 6 (PLANE) or
 *   count < 3 (POINT), or a pivot is <= 2^-40 times its original diagonal entry or is not finite: status |= PN2_ICP_SINGULAR,
 *   *err |= PN2_ICP_ERR_SINGULAR, x = 0, T and iters untouched.  A sum or an entry of T that is not finite: the same with
 *   PN2_ICP_ERR_NONFINITE in place of PN2_ICP_ERR_SINGULAR.
 * UPDATE.  w = x[0..2], v = x[3..5], th = sqrt((w_0 w_0 + w_1 w_1) + w_2 w_2), tt = th th.  a = sin(th) / th, b = (1 - cos(th)) / tt;
 *   below th = 2^-20: a = 1 - tt / 6, b = 1/2 - tt / 24.  K = [w]x, K2 = K K written out (K2_ii = -(w_j w_j + w_k w_k), j < k the
 *   other two; K2_ij = w_i w_j).  D = (I + a K) + b K2.  R <- D R, t <- D t + v, each entry a left-to-right sum of three products
 *   (+ v_i); iters += 1.  status |= PN2_ICP_CONVERGED iff th <= tol_rot and sqrt((v_0 v_0 + v_1 v_1) + v_2 v_2) <= tol_trans; the
 *   update of that step is applied.  (The linearisation rotates about the origin of the target frame: DESIGN.md, "ICP".)
 * PN2_ICP_EVAL_ONLY: sums, count and corr are written; no solve; T, x, status, iters are untouched and x / status / iters may be NULL.
 * PN2_EINVAL, nothing launched and nothing written: a null src / tgt / origin / cell / grid_workspace / T / sums / count / workspace
 * (x / status / iters without PN2_ICP_EVAL_ONLY), B < 1 or B > 65535, N < 1 or N > 2^31 - 256, M < 1 or M > PN2_VOXEL_MAX_ROWS, a pitch
 * outside 3..16, PN2_ICP_PLANE without normals, an unknown metric or flag, a negative or non-finite tolerance, a bad grid, a
 * misaligned pointer; pn2_icp_workspace_bytes returns PN2_EINVAL for such B / N. */
#define PN2_ICP_POINT 0
#define PN2_ICP_PLANE 1
#define PN2_ICP_EVAL_ONLY 1        /* flags: accumulate and write sums/count/corr; no solve, T, x, status, iters untouched */
#define PN2_ICP_CONVERGED 1        /* status bits */
#define PN2_ICP_SINGULAR  2
#define PN2_ICP_ERR_QUERY 1        /* err bits */
#define PN2_ICP_ERR_SINGULAR 2
#define PN2_ICP_ERR_NONFINITE 4
int64_t pn2_icp_workspace_bytes(int B, int N);
int pn2_icp_step(const float *src, int lds, int B, int N, const int64_t *n_src,
                 const float *tgt, int ldt, int M, const float *tgt_normal, int ldn,
                 const double *origin, const double *cell, const void *grid_workspace, float max_d2,
                 int metric, int flags, double tol_rot, double tol_trans,
                 double *T, double *sums, int64_t *count, double *x, int32_t *status, int32_t *iters,
                 int64_t *corr, int32_t *err, void *workspace, pn2_stream_t stream);

/* ---- plane RANSAC: the dominant plane of a cloud, its least-squares refit, height above it (csrc/plane.hip), added within ABI 15
 * (purely additive: no version change) ----------
 * pn2_plane_ransac scores H three-point hypotheses per cloud and selects one (three launches); pn2_plane_refit does ONE
 * least-squares round on that plane's inliers (two launches); pn2_plane_classify writes every row's signed distance, the inlier
 * count and the inliers' mark (two launches).  Plain launches on the caller's stream; no allocation, no host synchronisation, no
 * float atomics, no thread waits for another thread's write; the bytes are the same from run to run.  tests/plane_ref.py restates
 * the rule in numpy.
 *   pts [B,N,ld] fp32, 3 <= ld <= 16, columns 0..2 = x, y, z (a [., 4] scan is read where it lies).
 *   n_points  device int64 [B] or NULL (= N), clamped to [0,N]: n below.
 *   assign    device int32 [B,N] or NULL.  A row TAKES PART iff i < n and (assign is NULL or assign[b,i] < 0): planes are peeled off
 *             one after another by calling again on the same assign.
 *   axis      HOST double[3], finite, not zero; the entry point divides it by sqrt((a_x a_x + a_y a_y) + a_z a_z) in fp64.
 *   workspace pn2_plane_workspace_bytes(B, N, H) bytes of device memory, 16-byte aligned; it may hold anything before
 *             pn2_plane_ransac; pn2_plane_refit and pn2_plane_classify use a part of it whose place depends on (B, N) alone.
 * SAMPLER.  Hypothesis h < H of cloud b names rows row(0), row(1), row(2), a pure integer function, all arithmetic mod 2^64:
 *   x = seed * 0x9E3779B97F4A7C15 + (b << 40 | h << 8 | j);
 *   x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31;   row(j) = ((x >> 32) * n) >> 32.
 *   (This header is the definition, whatever generator the constants resemble.)
 * HYPOTHESIS, fp64, each operation rounded on its own, nothing fused.  p_j = double(pts[row(j)]).  INVALID if n = 0, two of the rows
 *   coincide, one takes no part, or one is not finite.  a = p_1 - p_0, b = p_2 - p_0, c = a x b componentwise
 *   (c_x = a_y b_z - a_z b_y, c_y = a_z b_x - a_x b_z, c_z = a_x b_y - a_y b_x), l2 = (c_x c_x + c_y c_y) + c_z c_z; INVALID unless
 *   l2 > 0 and finite; n = c / sqrt(l2) componentwise.  FLIP: with t = (n_x a_x + n_y a_y) + n_z a_z against the normalised axis, n is
 *   negated iff t < 0, or t == 0 and the first non-zero component of n is negative.  Then t is taken again; INVALID if t < cos_max.
 *   d = -((n_x p_0x + n_y p_0y) + n_z p_0z).  There is no retry: an invalid hypothesis is lost.
 * SCORE.  r = ((n_x x + n_y y) + n_z z) + d in fp64 with (x, y, z) = double(row).  A row is an INLIER iff it takes part, is finite and
 *   |r| <= threshold.  A row that takes part and is not finite sets PN2_PLANE_ERR_NONFINITE.  A hypothesis's score is its integer
 *   inlier count; hyp_count int32 [B,H] or NULL receives it, -1 for an invalid hypothesis.
 * SELECT.  The valid hypothesis with the largest count, the lowest h among equals: best_h int32 [B] (-1: no valid hypothesis),
 *   best_count int64 [B] (then 0), plane fp64 [B,4] = its (n_x, n_y, n_z, d) bit for bit, status int32 [B] = 0.  No valid hypothesis, or
 *   best_count < 3: plane = zeros, status = PN2_PLANE_NONE, *err |= PN2_PLANE_ERR_NONE, and pn2_plane_refit / pn2_plane_classify
 *   write nothing of that cloud.
 * REFIT (pn2_plane_refit, one round; callers run it `refine` times).  s = (-d) n, a point of the current plane.  Over the current
 *   plane's inliers, q = double(p) - s, ten fp64 sums: count, q_x, q_y, q_z, q_x q_x, q_x q_y, q_x q_z, q_y q_y, q_y q_z, q_z q_z ->
 *   sums fp64 [B,10] (each product rounded, then added).  The order of summation is a function of (B, N) alone and is not stated
 *   otherwise.  m = sum q / count;  C_ab = sum q_a q_b / count - m_a m_b;  (l0 <= l1 <= l2, u) = the eigenvalues and the
 *   eigenvector of l0 by csrc/sym_eig3.h (cyclic Jacobi, PN2_PCA_SWEEPS sweeps).  count < 3, or not l1 > 0, or u / l0 not finite:
 *   status |= PN2_PLANE_DEGENERATE, plane and rmse stay.  Otherwise n = u with the FLIP above,
 *   d = -((n_x (s_x + m_x) + n_y (s_y + m_y)) + n_z (s_z + m_z)), rmse[b] = sqrt(max(l0, 0)).  (No angle test: the refit of a
 *   plane that passed it moves by the noise.)
 * CLASSIFY (pn2_plane_classify).  With the plane as it stands: dist fp32 [B,N] or NULL, dist[b,i] = float(r) for EVERY row i < n,
 *   rows that take no part included -- the height above the plane along axis; NaN for a row that is not finite.  count int64 [B] =
 *   the inliers (among the rows that take part).  count < min_inliers: status |= PN2_PLANE_SMALL and assign is left alone;
 *   otherwise, where assign is given, assign = plane_id for the inliers.  Rows at and beyond n are not written.
 * PN2_EINVAL, nothing launched and nothing written: a null pts / plane / workspace / axis (ransac, refit) / required output, B < 1
 * or B > 65535, N < 1 or N > 2^31 - 256, H < 1 or H > 65536, a pitch outside 3..16, a threshold that is not finite and >= 0, a
 * cos_max that is not finite, an axis that is zero or not finite, plane_id < 0, a misaligned pointer (the workspace: 16 bytes);
 * pn2_plane_workspace_bytes returns PN2_EINVAL for such B / N / H. */
#define PN2_PLANE_NONE 1           /* status bits */
#define PN2_PLANE_DEGENERATE 2
#define PN2_PLANE_SMALL 4
#define PN2_PLANE_ERR_NONFINITE 1  /* err bits */
#define PN2_PLANE_ERR_NONE 2
int64_t pn2_plane_workspace_bytes(int B, int N, int H);
int pn2_plane_ransac(const float *pts, int ld, int B, int N, const int64_t *n_points, const int32_t *assign, int H, uint64_t seed,
                     const double *axis, double cos_max, double threshold, double *plane, int32_t *hyp_count, int32_t *best_h,
                     int64_t *best_count, int32_t *status, int32_t *err, void *workspace, pn2_stream_t stream);
int pn2_plane_refit(const float *pts, int ld, int B, int N, const int64_t *n_points, const int32_t *assign, const double *axis,
                    double threshold, double *plane, double *rmse, double *sums, int32_t *status, void *workspace, pn2_stream_t stream);
int pn2_plane_classify(const float *pts, int ld, int B, int N, const int64_t *n_points, int32_t *assign, int32_t plane_id,
                       int64_t min_inliers, double threshold, const double *plane, int32_t *status, float *dist, int64_t *count,
                       void *workspace, pn2_stream_t stream);

/* ---- FPFH: Fast Point Feature Histograms over neighbour lists (csrc/fpfh.hip), added within ABI 15 (purely additive: no version
 * change) ----------
 * 33 numbers per point, invariant to rigid motion (Rusu, Blodow, Beetz, ICRA 2009), from points, UNIT normals and a self-search's
 * "k nearest within r" lists.  pn2_spfh counts three angle bins per neighbour pair (integers); pn2_fpfh, after a launch boundary,
 * adds to every row's own histogram the 1 / d2 weighted mean of its neighbours' histograms.  One plain launch each on the caller's
 * stream; no allocation, no host synchronisation, no atomics except the OR into err, no thread waits for another; the bytes are
 * the same from run to run.  tests/fpfh_ref.py restates the rule in numpy.  THIS HEADER IS THE DEFINITION: it was written from the
 * paper and is UNVERIFIED AGAINST OPEN3D / PCL.  THE DESCRIPTOR DEPENDS ON THE SIGN OF THE NORMALS.
 *   points  [B,M,ldp] fp32, 3 <= ldp <= 16, columns 0..2 = x, y, z, read where they lie.
 *   normals [B,M,ldn] fp32, 3 <= ldn <= 16, the normal in columns normal_col .. normal_col + 2; it may be the points' buffer
 *           (a row x y z nx ny nz: ldn = 6, normal_col = 3).
 *   idx     [B,M,K] int64 as pn2_knn / pn2_grid_knn's self-search write it (padding: idx = M), 1 <= K <= 32.  Row i of idx belongs to
 *           point i: the search is a self-search.   max_d2 fp32, >= 0, +inf: no cut-off.
 *   n_points  device int64 [B] or NULL (= M), clamped to [0,M]: n below.  Rows at and beyond n are neither read nor written.
 * PAIR.  Slot s of row i with j = idx[i,s] is a PAIR iff, tested in this order,
 *   (G1) 0 <= j < n;
 *   (G2) p_i and p_j are finite; otherwise the slot is lost and *err |= PN2_FPFH_ERR_NONFINITE;
 *   (G3) with dp = double(p_j) - double(p_i) (exact), d2 = (dp.x*dp.x + dp.y*dp.y) + dp.z*dp.z:  0 < d2 <= double(max_d2)
 *        (the point itself and exact duplicates are not pairs);
 *   (N1) n_i and n_j are finite; otherwise the slot is lost and *err |= PN2_FPFH_ERR_NONFINITE (only a slot that passed G1..G3
 *        looks at the normals);
 *   (N2) neither normal is three zeros (pn2_local_pca's PN2_PCA_ERR_FEW rows: lost without a flag);
 *   (N3) |v| > 0 below.
 *   G1..G3 are the GEOMETRIC HALF of the test.  Nothing is poisoned; a candidate listed twice is two slots.
 * PAIR FEATURES, IEEE fp64, each operation rounded on its own, nothing fused; every dot product is (a.x*b.x + a.y*b.y) + a.z*b.z.
 *   d = sqrt(d2);  a1 = (n_i . dp) / d;  a2 = (n_j . dp) / d.
 *   If |a1| < |a2| the frame sits on j: n_s = n_j, n_t = n_i, dp = -dp, f3 = -a2.  Otherwise n_s = n_i, n_t = n_j, f3 = a1.
 *   (Open3D's acos(|a1|) > acos(|a2|) without the two acos calls: a stated deviation at ties.)
 *   v = dp x n_s  (v.x = dp.y n_s.z - dp.z n_s.y, v.y = dp.z n_s.x - dp.x n_s.z, v.z = dp.x n_s.y - dp.y n_s.x);  |v| = sqrt(v . v);
 *   v = v / |v| component by component;  w = n_s x v, the same way.
 *   f2 = v . n_t;   f1 = atan2((w . n_t) + 0.0, n_s . n_t)   (the + 0.0 turns -0 into +0: exactly antiparallel normals give +pi).
 *   t1 = 11.0 * (f1 + pi) / (2.0 * pi), left to right, pi = 3.14159265358979323846;  t2 = 11.0 * (f2 + 1.0) * 0.5;
 *   t3 = 11.0 * (f3 + 1.0) * 0.5;   b_k = floor(t_k) clamped to 0 .. 10 (a NaN: 0).
 *   The pair adds 1 to c_i[b_1], c_i[11 + b_2], c_i[22 + b_3] and to m_i.  atan2 is the one operation that is not correctly
 *   rounded everywhere: two implementations may differ on a pair whose t1 lies within a few 1e-15 of an integer.
 * SPFH ROW (pn2_spfh's output, a public intermediate): uint8 [B,M,36], 4-byte aligned: bytes 0..32 = c_i, byte 33 = m_i (both at
 *   most K <= 32), bytes 34..35 = 0.  m_i = 0: *err |= PN2_FPFH_ERR_EMPTY.
 * FPFH ROW (pn2_fpfh's output): fp32 [B,M,33].  IEEE fp64, ascending slot order, nothing fused.
 *   s_j[b] = (100.0 * c_j[b]) / m_j, 0 where m_j = 0.   Slot s of row i VOTES iff it passes G1..G3 (pn2_fpfh reads no normals; G2
 *   sets PN2_FPFH_ERR_NONFINITE here too) and m_j > 0.   W_i = sum of 1.0 / d2 and A_i[b] = sum of s_j[b] / d2 over the voting
 *   slots;   fpfh_i[b] = float(s_i[b] + (W_i > 0 ? A_i[b] / W_i : 0.0)).   m_i = 0: *err |= PN2_FPFH_ERR_EMPTY (the row then holds
 *   its neighbours' mean alone, or zeros).  Each third of a row with m_i > 0 and a voter sums to 200.
 * err: device int32, caller zeroes, may be NULL.
 * PN2_EINVAL, nothing launched and nothing written: a null points / normals / idx / spfh / output, B < 1 or B > 65535, M < 1 or
 * M > 2^31 - 256, K < 1, ldp or ldn outside 3..16, normal_col < 0 or normal_col + 3 > ldn, a negative or NaN max_d2, points / normals
 * / spfh / fpfh_out not 4-byte or idx not 8-byte aligned.  K > 32: PN2_EUNSUPPORTED, nothing launched. */
#define PN2_FPFH_ERR_EMPTY 1
#define PN2_FPFH_ERR_NONFINITE 2
int pn2_spfh(const float *points, int ldp, const float *normals, int ldn, int normal_col, const int64_t *idx, int B, int M, int K,
             float max_d2, const int64_t *n_points, uint8_t *spfh_out, int32_t *err, pn2_stream_t stream);
int pn2_fpfh(const float *points, int ldp, const int64_t *idx, const uint8_t *spfh, int B, int M, int K, float max_d2,
             const int64_t *n_points, float *fpfh_out, int32_t *err, pn2_stream_t stream);

/* ---- feature matching: the two nearest rows in feature space, mutual and ratio tests (csrc/feature_match.hip), added within ABI 15
 * (purely additive: no version change) ----------
 * pn2_feature_nn2 gives every query row its nearest and second-nearest candidate row (one launch); pn2_match_pairs filters one such
 * search, optionally against the search with the roles swapped, into a compacted pair list (four launches).  Plain launches on the
 * caller's stream; no allocation, no host synchronisation, no atomics, no thread waits for another thread's write; the bytes are
 * the same from run to run.  tests/match_ref.py restates the rule in numpy.
 *   query [B,N,ldq] fp32, cand [B,M,ldc] fp32; the feature is columns 0 .. D-1, 1 <= D <= PN2_MATCH_MAX_D, D <= ldq, D <= ldc (an
 *         FPFH row: D = ld = 33).
 *   n_query, n_cand  device int64 [B] or NULL (= N, M), clamped to [0,N] / [0,M], as in pn2_knn.
 * DISTANCE, fp32, each operation rounded on its own, nothing fused, in ascending c:  s = 0;  for c = 0 .. D-1: t = q[c] - f[c],
 *   s = s + t * t;  d2(i,j) = s.
 * TAKES PART.  A row (query or candidate) takes part iff its D values are all finite and not all zero (a row that pn2_fpfh flagged
 *   PN2_FPFH_ERR_EMPTY may hold zeros: left in, such rows would all match one another at distance 0).  A row that takes no part is
 *   never a candidate; as a query it gets idx = (M, M), dist = (+inf, +inf).
 * SELECT.  Among the candidates j < n_cand that take part, the two smallest by ascending (d2, j), every compare strict (pn2_knn's
 *   tie rule: equal distances keep their index order).  A NaN or +inf d2 is never kept.  idx int64 [B,N,2] (M: none), dist fp32
 *   [B,N,2] (+inf: none).  Rows at and beyond n_query are not written.
 * PAIRS (pn2_match_pairs).  idx / dist as above; back int64 [B,M,2] or NULL: the idx of the search with the roles swapped (mutual
 *   checking on).  Row i < n_query is KEPT iff, with j = idx[i,0]:  0 <= j < M;  back is NULL or back[j,0] == i;  and
 *   ratio2 == +inf, or dist[i,1] == +inf (no second neighbour), or dist[i,0] <= ratio2 * dist[i,1] (one fp32 multiply).
 *   The kept rows are written in ascending i: pair_src int64 [B,N] = i, pair_tgt int64 [B,N] = j, count int64 [B]; entries at and
 *   beyond count are not written.  workspace: pn2_match_pairs_workspace_bytes(B, N) bytes, 16-byte aligned, may hold anything.
 * PN2_EINVAL, nothing launched and nothing written: a null query / cand / idx / dist / pair list / count / workspace, B < 1 or
 * B > 65535, N or M < 1 or > 2^31 - 256, D < 1 or above a pitch, a ratio2 that is negative or NaN, a misaligned pointer (floats 4,
 * int64 8, the workspace 16 bytes).  D > PN2_MATCH_MAX_D: PN2_EUNSUPPORTED, nothing launched. */
#define PN2_MATCH_MAX_D 64
int pn2_feature_nn2(const float *query, int ldq, const float *cand, int ldc, int B, int N, int M, int D, const int64_t *n_query,
                    const int64_t *n_cand, int64_t *idx, float *dist, pn2_stream_t stream);
int64_t pn2_match_pairs_workspace_bytes(int B, int N);
int pn2_match_pairs(const int64_t *idx, const float *dist, const int64_t *back, int B, int N, int M, float ratio2, const int64_t *n_query,
                    int64_t *pair_src, int64_t *pair_tgt, int64_t *count, void *workspace, pn2_stream_t stream);

/* ---- correspondence RANSAC: the rigid transform of a pair list, and its least-squares refit (csrc/corr_ransac.hip), added within
 * ABI 15 (purely additive: no version change) ----------
 * pn2_corr_ransac scores H three-pair hypotheses per cloud and selects one (three launches); pn2_corr_refit does ONE least-squares
 * round on that transform's inliers (two launches).  Plain launches on the caller's stream; no allocation, no host synchronisation,
 * no float atomics, no thread waits for another thread's write; the bytes are the same from run to run.
 * tests/corr_ransac_ref.py restates the rule in numpy.  IEEE fp64 throughout, each operation rounded on its own, nothing fused.
 *   src [B,N,lds], tgt [B,M,ldt] fp32, 3 <= ld <= 16, columns 0..2 = x, y, z, read where they lie.
 *   pair_src, pair_tgt  int64 [B,N]: pair k of cloud b joins source row pair_src[b,k] and target row pair_tgt[b,k] (pn2_match_pairs'
 *             output).   count  device int64 [B] or NULL (= N), clamped to [0,N]: n below.
 *   T         fp64 [B,12] = [R | t] row major (T[4a + c] = R_ac, T[4a + 3] = t_a): pn2_icp_step's layout.
 *   workspace pn2_corr_workspace_bytes(B, N, H) bytes of device memory, 16-byte aligned; it may hold anything before
 *             pn2_corr_ransac; pn2_corr_refit uses a part of it whose place depends on (B, N) alone.
 * HYPOTHESIS h < H: pair rows r_j = row(j), j = 0, 1, 2, by the SAMPLER of "plane RANSAC" above among n rows;
 *   a_j = double(src[pair_src[r_j]]), b_j = double(tgt[pair_tgt[r_j]]).  INVALID if n < 3; two of the r_j, of the source indices
 *   or of the target indices coincide; an index lies outside [0,N) / [0,M); one of the six points is not finite; for one of the
 *   edges (0,1), (0,2), (1,2) the lengths lp = |a_j - a_i|, lq = |b_j - b_i| (|d| = sqrt((d_x d_x + d_y d_y) + d_z d_z)) do not
 *   satisfy lp > 0, lq > 0 and min(lp, lq) >= edge_ratio * max(lp, lq);  a frame below has |w| = 0 or not finite;  or one of the
 *   twelve results is not finite.  There is no retry: an invalid hypothesis is lost (twelve NaNs in hyp_T).
 *   FRAME of a side (a_0, a_1, a_2):  e1 = (a_1 - a_0) / |a_1 - a_0|;  v = a_2 - a_0;  w = e1 x v componentwise (w_x = e1_y v_z -
 *   e1_z v_y, w_y = e1_z v_x - e1_x v_z, w_z = e1_x v_y - e1_y v_x);  e3 = w / |w|;  e2 = e3 x e1 the same way;
 *   c = ((a_0 + a_1) + a_2) / 3.0.   With (e1, e2, e3, c) of the source side and (f1, f2, f3, c') of the target side:
 *   R_ac = (f1_a e1_c + f2_a e2_c) + f3_a e3_c;   t_a = c'_a - ((R_a0 c_x + R_a1 c_y) + R_a2 c_z).
 * SCORE.  For pair k < n with p = double(src row), q = double(tgt row): e_a = (((R_a0 p_x + R_a1 p_y) + R_a2 p_z) + t_a) - q_a,
 *   d2 = (e_x e_x + e_y e_y) + e_z e_z; the pair is an INLIER iff both indices are in range, both points are finite and
 *   d2 <= threshold * threshold (the product rounded once).  An index out of range sets PN2_CORR_ERR_PAIR, a point that is not
 *   finite PN2_CORR_ERR_NONFINITE.  hyp_count int32 [B,H] or NULL receives every hypothesis's inlier count, -1 for an invalid one;
 *   hyp_T fp64 [B,H,12] or NULL its twelve doubles.
 * SELECT.  The valid hypothesis with the largest count, the lowest h among equals: best_h int32 [B] (-1: none valid), best_count
 *   int64 [B] (then 0), T = its twelve doubles bit for bit, status int32 [B] = 0.  No valid hypothesis, or best_count < 3: T = the
 *   identity, status = PN2_CORR_NONE, *err |= PN2_CORR_ERR_NONE, and pn2_corr_refit writes nothing of that cloud.
 * REFIT (pn2_corr_refit, one round; callers run it `refine` times).  Over the inliers of the current T, PN2_CORR_SUMS = 17 fp64
 *   sums -> sums [B,17]: count; p_x, p_y, p_z; q_x, q_y, q_z; p_a q_b for (a, b) = (x,x), (x,y), (x,z), (y,x), ... (z,z) (each
 *   product rounded, then added); d2.  The order of summation is a function of (B, N) alone and is not stated otherwise.
 *   inliers int64 [B] = count;  rmse fp64 [B] = sqrt(sum d2 / count), 0 for count = 0: the root mean square distance of the inliers
 *   UNDER THE T THE ROUND STARTED FROM.  With flags = PN2_CORR_EVAL_ONLY the round ends here.  Otherwise (Horn 1987), n = count:
 *   S_ab = sum p_a q_b - (sum p_a * sum q_b) / n;
 *   N00 = (S_xx + S_yy) + S_zz, N11 = (S_xx - S_yy) - S_zz, N22 = (S_yy - S_xx) - S_zz, N33 = (S_zz - S_xx) - S_yy,
 *   N01 = S_yz - S_zy, N02 = S_zx - S_xz, N03 = S_xy - S_yx, N12 = S_xy + S_yx, N13 = S_zx + S_xz, N23 = S_yz + S_zy;
 *   u = the eigenvector of N's largest eigenvalue by csrc/sym_eig4.h (cyclic Jacobi, pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3),
 *   PN2_HORN_SWEEPS = 8 sweeps, the largest diagonal entry, the first among equals);  (w, x, y, z) = u / sqrt(((u_0 u_0 + u_1 u_1)
 *   + u_2 u_2) + u_3 u_3), negated iff w < 0;
 *   R_00 = ((w w + x x) - y y) - z z, R_01 = 2 (x y - w z), R_02 = 2 (x z + w y), R_10 = 2 (x y + w z), R_11 = ((w w - x x) + y y)
 *   - z z, R_12 = 2 (y z - w x), R_20 = 2 (x z - w y), R_21 = 2 (y z + w x), R_22 = ((w w - x x) - y y) + z z;
 *   t_a = (sum q_a) / n - ((R_a0 m_x + R_a1 m_y) + R_a2 m_z) with m = (sum p) / n.   (The quaternion route handles inliers that
 *   lie in a plane, S of rank 2, and never returns a reflection.)   n < 3, or a result that is not finite: status |=
 *   PN2_CORR_DEGENERATE and T stays.
 * err: device int32, caller zeroes, may be NULL.
 * PN2_EINVAL, nothing launched and nothing written: a null src / tgt / pair list / T / workspace / required output, B < 1 or
 * B > 65535, N or M < 1 or > 2^31 - 256, H < 1 or H > 65536, a pitch outside 3..16, a threshold that is not finite and >= 0, an
 * edge_ratio outside [0,1], unknown flags, a misaligned pointer (the workspace: 16 bytes); pn2_corr_workspace_bytes returns
 * PN2_EINVAL for such B / N / H. */
#define PN2_CORR_NONE 1            /* status bits */
#define PN2_CORR_DEGENERATE 2
#define PN2_CORR_ERR_PAIR 1        /* err bits */
#define PN2_CORR_ERR_NONFINITE 2
#define PN2_CORR_ERR_NONE 4
#define PN2_CORR_EVAL_ONLY 1       /* pn2_corr_refit's flag */
#define PN2_CORR_SUMS 17
int64_t pn2_corr_workspace_bytes(int B, int N, int H);
int pn2_corr_ransac(const float *src, int lds, const float *tgt, int ldt, int B, int N, int M, const int64_t *pair_src, const int64_t *pair_tgt,
                    const int64_t *count, int H, uint64_t seed, double edge_ratio, double threshold, double *T, double *hyp_T,
                    int32_t *hyp_count, int32_t *best_h, int64_t *best_count, int32_t *status, int32_t *err, void *workspace,
                    pn2_stream_t stream);
int pn2_corr_refit(const float *src, int lds, const float *tgt, int ldt, int B, int N, int M, const int64_t *pair_src, const int64_t *pair_tgt,
                   const int64_t *count, double threshold, int flags, double *T, int64_t *inliers, double *rmse, double *sums,
                   int32_t *status, void *workspace, pn2_stream_t stream);

/* ---- voxel-grid downsampling (csrc/voxel.hip), added within ABI 15 (purely additive: no version change) ------------------------------
 * One row per occupied cell of a regular grid, for a batch of B clouds that lie back to back in device memory (the conventions
 * of pn2_scan_filter: device-side row_begin / row_count / out_begin, a host bound max_rows that sizes the grid of workgroups and
 * the workspace only).  At most six plain launches on the caller's stream; no host synchronisation, no allocation, no thread
 * waits for another thread's write.
 *   pts        [rows, ld] fp32, 3 <= ld <= 16, columns 0..2 = x, y, z; cloud b is rows [row_begin[b], row_begin[b] + row_count[b]).
 *   labels_in  int32[rows] or NULL (out_labels then holds zeros).
 *   max_rows   host upper bound of every row_count[b], 0 <= max_rows <= PN2_VOXEL_MAX_ROWS (2^29 rows per cloud).  Tiles of
 *              PN2_VOXEL_TILE rows that start at or beyond the device-side row_count[b] do nothing, so a captured launch stays
 *              valid when the count changes.  A negative row_count counts as 0.
 *   origin, voxel   HOST double[3] each: voxel[a] finite and > 0, origin[a] finite (else PN2_EINVAL, nothing launched).
 *   out_begin  int64[B] (device): where cloud b's voxels start in the outputs.  Outputs must not alias inputs.
 * THE RULE, per row and per axis a:
 *   q_a = floor(((double)p_a - origin[a]) / voxel[a])      IEEE fp64, each operation rounded on its own.
 *   The row is VALID iff q_a >= -1048576.0 && q_a < 1048576.0 for all three axes, compared in fp64 before any conversion to an
 *   integer (NaN and +-inf fail).  An invalid row is dropped, gets inverse = -1 and sets PN2_VOXEL_ERR_RANGE.  -0.0 lies in cell 0.
 *   key = (q_x + 2^20) << 42 | (q_y + 2^20) << 21 | (q_z + 2^20): three biased 21-bit integers in 63 bits.
 *   Valid rows of ONE cloud with equal keys form a voxel (clouds never share voxels, even at equal coordinates).  A voxel's
 *   representative is its row with the lowest row number inside the cloud.  The representatives come in ascending row number:
 *   a STABLE compaction, np.sort(np.unique(key, return_index=True)[1]).
 * Outputs, for rank r = 0 .. out_count[b] - 1 of cloud b at position out_begin[b] + r (each may be NULL except out_count):
 *   out_points fp32 [., ld]  the representative's row, all ld floats bit for bit;   out_labels int32  its label;
 *   out_index  int32         its row inside the cloud, strictly increasing;         n_points   int32  valid rows in the voxel;
 *   inverse    int32[rows]   inverse[row_begin[b] + i] = the rank, inside cloud b, of row i's voxel (-1: invalid row); rows outside
 *                            the clouds are not written;                            out_count  int64[B]  the number of voxels.
 *   Everything is the same from run to run, byte for byte: a lock-free hash table driven by integer atomics (64-bit
 *   compare-and-swap on the key, minimum of the row number, sum of the population) decides WHICH rows stand for their voxels,
 *   prefix sums decide WHERE they go; neither the hash function nor the probe order shows in any output.
 * err (device int, caller zeroes, may be NULL) receives
 *   PN2_VOXEL_ERR_RANGE  a row with a non-finite coordinate or a cell outside [-2^20, 2^20): dropped;
 *   PN2_VOXEL_ERR_ROWS   a row_count[b] above max_rows: the rows beyond are ignored.
 * workspace: pn2_voxel_grid_workspace_bytes(B, max_rows) bytes of device memory, 16-byte aligned; it may hold anything on entry
 * and its content need not be kept (per cloud: a table of the power of two >= 2 * max_rows slots of 16 bytes, and 5 bytes per row).
 * PN2_EINVAL without a launch for a null pts / row_begin / row_count / origin / voxel / out_begin / out_count / workspace, B < 1 or
 * B > 65535, max_rows < 0 or > PN2_VOXEL_MAX_ROWS, ld outside 3..16, pts / out_points not 4-byte or workspace not 16-byte aligned;
 * pn2_voxel_grid_workspace_bytes returns PN2_EINVAL for such B / max_rows.  (ld == 4 with 16-byte aligned pts and out_points
 * moves rows as 16-byte words.) */
#define PN2_VOXEL_TILE 1024
#define PN2_VOXEL_MAX_ROWS ((int64_t)1 << 29)
#define PN2_VOXEL_ERR_RANGE 1
#define PN2_VOXEL_ERR_ROWS 2
int64_t pn2_voxel_grid_workspace_bytes(int B, int64_t max_rows);
int pn2_voxel_grid(const float *pts, int ld, const int32_t *labels_in, const int64_t *row_begin, const int64_t *row_count, int B,
                   int64_t max_rows, const double *origin, const double *voxel, const int64_t *out_begin, float *out_points,
                   int32_t *out_labels, int32_t *out_index, int64_t *out_count, int32_t *inverse, int32_t *n_points, int *err,
                   void *workspace, pn2_stream_t stream);

/* ---- segment reductions: voxel mean, its backward pass, majority label (csrc/voxel_reduce.hip), added within ABI 15 (additive) ------
 * Reductions over an `inverse`-style map, as pn2_voxel_grid writes it.  SEGMENTS are what pn2_voxel_grid calls voxels:
 *   row row_begin[b] + i of cloud b (i < row_count[b]) belongs to output row out_begin[b] + seg[row_begin[b] + i];
 *   seg         int32[rows]: the rank of the row's segment inside its cloud.  A NEGATIVE seg: the row takes no part.  A seg at or
 *               beyond out_count[b] or max_rows: the row takes no part either and sets PN2_SEGMENT_ERR_RANGE; it never causes a
 *               write outside the cloud's output range;
 *   out_count   int64[B] (DEVICE): the segments of cloud b.  Output rows at or beyond it are not written;
 *   row_begin, row_count, max_rows, out_begin follow pn2_voxel_grid; every count is read on the device and clamped to
 *               [0, max_rows], so a captured call stays valid when the counts change.
 * Plain launches on the caller's stream (mean 4, backward 1, mode 4); no host synchronisation, no allocation, no thread waits for
 * another thread's write.  Everything that crosses threads is an integer atomic (max, add, compare-and-swap): integer maxima and
 * sums commute, so every output is the same from run to run, byte for byte, whatever the order of the rows' arrival.
 *
 * THE MEAN, per segment and per column c < C (1 <= C <= PN2_SEGMENT_MAX_COLS; values fp32 of pitch ld >= C, out of pitch ld_out >= C):
 *   1. a finite float32 is s * M * 2^(k - 150): for an exponent field e >= 1, M = 2^23 + fraction and k = e; for e = 0, M = fraction
 *      and k = 1.  K is the largest k among the segment's terms in that column.
 *   2. a term contributes the integer t = s * ((M << 10) >> (K - k)): the shift truncates the magnitude, t = 0 when K - k >= 34.
 *      |t| < 2^34 and at most 2^29 rows: S = sum of t fits a signed 64-bit word exactly, whatever the order.
 *   3. mean = float32(ldexp(double(S) / double(n), K - 160)): int64 -> fp64 to nearest even, ONE IEEE fp64 division, an exact
 *      power-of-two scaling in fp64, ONE rounding to float32 (subnormal results included).  n is the number of rows that take part:
 *      n_points[out row] (int32, e.g. pn2_voxel_grid's) or, with n_points NULL, counted by the call.  n_out (int32, may be NULL)
 *      receives the n that was used.  A given n_points <= 0 gives +0.0.
 *   4. a NaN or +-inf term: the column's mean is the quiet NaN 0x7FC00000 and PN2_SEGMENT_ERR_NONFINITE is set (a stated deviation:
 *      numpy gives +-inf for infinities of one sign); the segment's other columns are not affected.
 *   5. a segment without rows gives +0.0 (and S = 0 gives +0.0: x and -x cancel exactly).
 *   Every term is truncated by less than one unit 2^(K - 160), at most 2^-33 of the column's largest magnitude, so
 *   |mean - exact mean| <= 2^(K - 160) + 1/2 ulp32(mean) + |exact| * 2^-51; sums that would overflow float32 do not overflow here.
 * THE MEAN, BACKWARD: grad_in[row, c] = grad_out[out_begin[b] + seg[row], c] / float(n_points[out row]), one IEEE float32 division;
 *   a row that takes no part gets +0.0 (and so does a row whose n_points is <= 0); rows outside the clouds are not written.
 * THE MAJORITY LABEL: a row votes iff it takes part and its int32 label is >= 0.  The label with the most votes wins, among equals
 *   the LOWEST label; a segment with no voter gets `fill`.  votes (int32, may be NULL) receives the winner's count (0: no voter);
 *   votes / n_points is the cell's purity.  No class limit: any label up to 2^31 - 1.  (out_labels may be NULL when votes is not.)
 * err (device int, caller zeroes, may be NULL) receives PN2_SEGMENT_ERR_RANGE and PN2_SEGMENT_ERR_NONFINITE; the bits are disjoint
 * from PN2_VOXEL_ERR_*, so one word can serve a pn2_voxel_grid call and the reductions that follow it.
 * workspace: pn2_segment_reduce_workspace_bytes(B, max_rows, C) bytes of device memory, 16-byte aligned, enough for EITHER
 * pn2_segment_mean with up to C columns OR pn2_segment_mode (calls on one stream may share it); it may hold anything on entry.
 * Per cloud: 12 bytes per (row, column) + 4 per row for the mean; a table of the power of two >= 2 * max_rows 16-byte slots + 8 bytes
 * per row for the mode.
 * PN2_EINVAL without a launch: a null required pointer, C outside 1..16, ld / ld_out / ld_in < C, B < 1 or B > 65535, max_rows < 0
 * or > PN2_VOXEL_MAX_ROWS, a pointer that is not 4-byte (workspace: 16-byte) aligned; pn2_segment_reduce_workspace_bytes returns
 * PN2_EINVAL for such B / max_rows / C. */
#define PN2_SEGMENT_MAX_COLS 16
#define PN2_SEGMENT_ERR_RANGE 4
#define PN2_SEGMENT_ERR_NONFINITE 8
int64_t pn2_segment_reduce_workspace_bytes(int B, int64_t max_rows, int C);
int pn2_segment_mean(const float *values, int ld, int C, const int32_t *seg, const int64_t *row_begin, const int64_t *row_count, int B,
                     int64_t max_rows, const int64_t *out_begin, const int64_t *out_count, const int32_t *n_points, float *out, int ld_out,
                     int32_t *n_out, int *err, void *workspace, pn2_stream_t stream);
int pn2_segment_mean_bwd(const float *grad_out, int ld_out, int C, const int32_t *seg, const int64_t *row_begin, const int64_t *row_count,
                         int B, int64_t max_rows, const int64_t *out_begin, const int64_t *out_count, const int32_t *n_points,
                         float *grad_in, int ld_in, int *err, pn2_stream_t stream);
int pn2_segment_mode(const int32_t *labels, const int32_t *seg, const int64_t *row_begin, const int64_t *row_count, int B, int64_t max_rows,
                     const int64_t *out_begin, const int64_t *out_count, int32_t fill, int32_t *out_labels, int32_t *votes, int *err,
                     void *workspace, pn2_stream_t stream);

/* ---- Euclidean clustering on the voxel grid (csrc/voxel_cluster.hip), added within ABI 15 (purely additive: no version change) ---------
 * Connected components of the occupied cells of a pn2_voxel_grid result: an instance id for every voxel and every row.  B clouds in
 * that call's conventions (device-side row_begin / row_count for the rows, out_begin / out_count for the voxels, a host bound
 * max_rows of both; every count is read on the device and clamped to [0, max_rows]).  At most eight plain launches on the caller's
 * stream sized by max_rows; no host synchronisation, no allocation, no thread waits for another thread's write.
 *   pts, ld, origin, voxel   as pn2_voxel_grid took them;
 *   out_index  int32  per voxel: its representative row inside the cloud;     n_points  int32 per voxel: its rows;
 *   vox_labels int32  per voxel or NULL;        inverse  int32 per row (needed for row_component);      row_labels  int32 per row or NULL
 *              (needs vox_labels);              member   int32[L] on the device or NULL (needs vox_labels and L >= 1).
 * THE RULE.
 *   CELL.  A voxel's cell is the cell of its representative row under pn2_voxel_grid's rule (fp64, each operation rounded on its own).
 *   TAKING PART.  A voxel takes part iff vox_labels is NULL, or vox_labels[v] >= 0 and member is NULL, or vox_labels[v] >= 0 and
 *     member[vox_labels[v]] != 0.  A label at or beyond L takes no part and raises no error.
 *   ADJACENCY.  Two voxels of ONE cloud are adjacent iff both take part and their cells differ by a vector d in {-1,0,1}^3 \ {0} with at
 *     most 1 (connectivity 6), 2 (18) or 3 (26) non-zero entries; with same_label != 0 and vox_labels given their labels must be equal
 *     too.  A neighbour cell exists only if -2^20 <= q_a + d_a < 2^20 on every axis, checked per axis before a key is formed: the
 *     cells at the two ends of an axis are no neighbours.  Clouds never share components.
 *   COMPONENTS.  A component is a connected component of that graph.  Its ROOT is its lowest voxel rank (also its lowest row: ranks
 *     ascend with the row), its points the sum of n_points over its voxels, its voxels their number, its label the root's label (0
 *     without vox_labels).  It is KEPT iff points >= min_points and voxels >= min_voxels (host ints >= 1).
 *   IDS.  The kept components of cloud b get the ids 0 .. comp_count[b] - 1 in ASCENDING ORDER OF THEIR ROOT: a stable compaction.
 * Outputs (each may be NULL except comp_count; rows and voxels outside the clouds' ranges are not written):
 *   vox_component int32 per voxel (at out_begin[b] + v): the id, -1 for "takes no part" or "component not kept";
 *   row_component int32 per row: -1 when inverse < 0, else the voxel's id; with row_labels, a row whose label differs from its voxel's
 *                 label gets -1.  An `inverse`-style map: pn2_segment_mean / pn2_segment_mode reduce over it with comp_count;
 *   comp_root (the root's voxel rank), comp_points, comp_voxels, comp_label   int32 per component at comp_begin[b] + id;
 *   comp_count    int64[B], left on the device.
 *   Everything is the same from run to run, byte for byte.  Which voxel links to which in the lock-free forest depends on the
 *   schedule; what is written does not: the partition is a property of the graph, a root is the minimum rank of its part, the counters
 *   are integer sums and the ids are prefix sums over ranks.
 * err (device int, caller zeroes, may be NULL) receives bits disjoint from PN2_VOXEL_ERR_* and PN2_SEGMENT_ERR_*:
 *   PN2_CLUSTER_ERR_INDEX  an out_index outside the cloud's rows (the voxel takes no part) or an inverse at or beyond the voxel count
 *                          (the row gets -1): skipped, never addressed;
 *   PN2_CLUSTER_ERR_CELL   a representative row whose cell is invalid: the voxel takes no part;
 *   PN2_CLUSTER_ERR_CAP    a walk of the forest took more steps than the cloud has voxels (cannot happen: entries only decrease); the
 *                          thread stopped, the result is not to be used;
 *   PN2_CLUSTER_ERR_ROWS   an out_count[b] (or, with row_component, a row_count[b]) above max_rows: what lies beyond is ignored.
 * workspace: pn2_voxel_components_workspace_bytes(B, max_rows) bytes of device memory, 16-byte aligned; it may hold anything on entry
 * (per cloud: a table of the power of two >= 2 * max_rows slots of 16 bytes, and 25 bytes per voxel).
 * PN2_EINVAL without a launch: a null pts / row_begin / row_count / origin / voxel / out_begin / out_count / out_index / n_points /
 * comp_begin / comp_count / workspace, B < 1 or B > 65535, max_rows < 0 or > PN2_VOXEL_MAX_ROWS, ld outside 3..16, a connectivity
 * other than 6, 18, 26, min_points < 1, min_voxels < 1, member without vox_labels or with L < 1, row_labels without vox_labels,
 * row_component without inverse, a voxel size that is not finite and > 0, an origin that is not finite, pts not 4-byte or workspace
 * not 16-byte aligned; pn2_voxel_components_workspace_bytes returns PN2_EINVAL for such B / max_rows. */
#define PN2_CLUSTER_ERR_INDEX 16
#define PN2_CLUSTER_ERR_CELL 32
#define PN2_CLUSTER_ERR_CAP 64
#define PN2_CLUSTER_ERR_ROWS 128
int64_t pn2_voxel_components_workspace_bytes(int B, int64_t max_rows);
int pn2_voxel_components(const float *pts, int ld, const int64_t *row_begin, const int64_t *row_count, int B, int64_t max_rows,
                         const double *origin, const double *voxel, const int64_t *out_begin, const int64_t *out_count,
                         const int32_t *out_index, const int32_t *n_points, const int32_t *vox_labels, const int32_t *inverse,
                         const int32_t *row_labels, int connectivity, int same_label, const int32_t *member, int L, int min_points,
                         int min_voxels, const int64_t *comp_begin, int32_t *vox_component, int32_t *row_component, int32_t *comp_root,
                         int32_t *comp_points, int32_t *comp_voxels, int32_t *comp_label, int64_t *comp_count, int *err, void *workspace,
                         pn2_stream_t stream);

/* ---- segment boxes: an oriented bounding box per segment, an L-shape fit swept by angle (csrc/boxes.hip), added within ABI 15
 * (purely additive: no version change) ------------------------------------------------------------------------------------------------
 * Length, width, height and heading of every segment of an `inverse`-style map: pn2_voxel_components' row_component / comp_count
 * (an instance's box), pn2_voxel_grid's inverse / out_count, or any other.  The reference has no such function.  tests/box_ref.py
 * restates the rule in numpy.  Every output is an integer, a minimum or a maximum (or one fixed chain of float32 operations on
 * those), so the bytes depend neither on the order of the rows nor on which thread saw which row.
 * SEGMENTS are pn2_segment_mean's, unchanged: seg int32 per row, a NEGATIVE seg takes no part; a seg at or beyond the device-side
 *   out_count[b] (clamped to max_rows) takes no part and sets PN2_BOX_ERR_RANGE; row_begin / row_count / max_rows / out_begin /
 *   out_count mean what they mean there, every count is read on the device and clamped to [0, max_rows].
 * COLUMNS.  pts is float32 of pitch ld; three DISTINCT column indices cx, cy, cz < ld name the two ground-plane coordinates and the
 *   height ((0, 1, 2): KITTI's z-up).
 * TAKING PART.  A row of a segment takes part iff its three values are finite and |x|, |y| <= 2^60.  Any other row of a segment takes
 *   no part and sets PN2_BOX_ERR_NONFINITE (a stated choice: a box with one NaN row left out is more use than a NaN box; the
 *   magnitude cut removes every overflow from the arithmetic below).  Rows with a negative or out-of-range seg are not looked at.
 * ANGLE TABLE.  angles: float32 [A, 4] on the device, (c_a, s_a, yaw_a, 0), 1 <= A <= PN2_BOX_MAX_ANGLES.  The kernels do no
 *   trigonometry: the caller fills the table (pointnet12_amd/boxes.py: theta_a = a * (pi / 2) / A in fp64, c = float32(cos theta),
 *   s = float32(sin theta), yaw = float32(theta)).
 * PROJECTION, per row and angle, float32, every operation rounded on its own:  u = (c*x) + (s*y),  v = (c*y) - (s*x).
 * EXTENT.  u0, u1, v0, v1: the minimum and maximum of u and of v over the segment's rows IN THE TOTAL ORDER OF THE ORDER-PRESERVING
 *   uint32 KEY (bits | 0x80000000 for a clear sign bit, ~bits otherwise: -0.0 < +0.0).  The same order gives z0, z1 of the height column
 *   and the raw box lo[3], hi[3] (of cx, cy, cz).  lu = u1 - u0, lv = v1 - v0, area = lu * lv.
 * SCORE (the closeness criterion of Zhang et al., "Efficient L-shape fitting for vehicle detection using laser scanners", IV 2017,
 *   quantised).  d0 float32, finite; d0 <= 0 means AREA ONLY: the score of every angle is 0.  Otherwise, per row and angle:
 *     e = fminf(fminf(u - u0, u1 - u), fminf(v - v0, v1 - v));  d = fmaxf(e, d0);  q = d0 / d (one IEEE float32 division);
 *     t = (int32)(q * 1048576.0f) (an exact product, truncated: 0 <= t <= 2^20);  score_a = sum of t in int64 (at most 2^29 rows: exact).
 * SELECTION.  The angle with the largest score wins, among equal scores the smaller area (float32 <), among equal areas the LOWEST a.
 * OUTPUTS, per segment s of cloud b at row out_begin[b] + s (center, size, lo, hi: three floats per row):
 *   angle  int32, -1 for a segment without rows;      yaw = yaw_a;      size = (lu, lv, z1 - z0);
 *   center: cu = 0.5f * (u0 + u1), cv = 0.5f * (v0 + v1), x = (c*cu) - (s*cv), y = (s*cu) + (c*cv), z = 0.5f * (z0 + z1);
 *   lo, hi; n int32: the rows that took part; score int64.
 *   A segment without rows writes +0.0 / -1 / 0.  Output rows at or beyond out_count[b] are not written.  angle, lo, hi, n and score
 *   may each be NULL.
 * Six plain launches on the caller's stream sized by max_rows (csrc/boxes.hip: rows bucketed by segment through an integer cursor,
 * then one angle per lane); no allocation, no host synchronisation, no float atomics, no thread waits for another thread's write.
 * A segment with at least split_rows rows (0: the default, 4096; otherwise 64 .. PN2_VOXEL_MAX_ROWS) is swept by a workgroup of 16 waves
 * instead of one wave; THE BYTES ARE THE SAME whichever serves it, and from run to run.
 * err (device int, caller zeroes, may be NULL) receives PN2_BOX_ERR_RANGE and PN2_BOX_ERR_NONFINITE; the bits are disjoint from
 * PN2_VOXEL_ERR_*, PN2_SEGMENT_ERR_*, PN2_CLUSTER_ERR_* and PN2_PANOPTIC_ERR_*: one word serves a downsample -> cluster -> boxes chain.
 * workspace: pn2_segment_boxes_workspace_bytes(B, max_rows) bytes of device memory (16 per row and 4 per cloud, rounded), 16-byte
 * aligned; it may hold anything on entry.
 * PN2_EINVAL without a launch: a null pts / seg / row_begin / row_count / out_begin / out_count / angles / center / size / yaw /
 * workspace, A outside 1..256, columns that are not distinct or not below ld, B < 1 or B > 65535, max_rows < 0 or >
 * PN2_VOXEL_MAX_ROWS, a split_rows other than 0 or 64 .. PN2_VOXEL_MAX_ROWS, a d0 that is not finite, a pointer that is not 4-byte
 * (score: 8-byte; angles, workspace: 16-byte) aligned; pn2_segment_boxes_workspace_bytes returns PN2_EINVAL for such B / max_rows. */
#define PN2_BOX_MAX_ANGLES 256
#define PN2_BOX_ERR_RANGE 1024
#define PN2_BOX_ERR_NONFINITE 2048
int64_t pn2_segment_boxes_workspace_bytes(int B, int64_t max_rows);
int pn2_segment_boxes(const float *pts, int ld, int cx, int cy, int cz, const int32_t *seg, const int64_t *row_begin, const int64_t *row_count,
                      int B, int64_t max_rows, const int64_t *out_begin, const int64_t *out_count, const float *angles, int A, float d0,
                      int split_rows, float *center, float *size, float *yaw, int32_t *angle, float *lo, float *hi, int32_t *n,
                      int64_t *score, int *err, void *workspace, pn2_stream_t stream);

/* ---- camera colour lookup for points (csrc/image.hip), added within ABI 15 (purely additive: no version change) -------------------
 * pn2_sample_image writes the colour of the pixel under each projected point: the per-point loop of
 * data_utils/ColorGenerator_Loader.py:63-65 (`pts_color[i] = frame_HSV[row, col]` inside the frame) and the divisions of :68-69, for
 * a batch of B clouds whose rows lie back to back in device memory.  One plain launch; no host synchronisation, no allocation.
 *   pix        int32 [rows, 2] (8-byte aligned), exactly what pn2_project_points writes: x = column, y = row, INT32_MIN in both
 *              for an unprojectable point.
 *   image      uint8 [B, H, W, 3], contiguous, device memory; cloud b reads image b only.  H * W * 3 < 2^31 per image.
 *   channel_order  PN2_CHANNELS_RGB: the bytes of a pixel are R, G, B; PN2_CHANNELS_BGR: B, G, R (a cv2.imread frame, read in place).
 *   mode / normalize   PN2_IMAGE_RGB or PN2_IMAGE_HSV; 0 or 1.
 *   row_begin, row_count   int64[B], DEVICE memory, with the host bound max_rows (0 <= max_rows < 2^31): pn2_scan_filter's
 *              conventions.  Cloud b is rows [row_begin[b], row_begin[b] + min(max(row_count[b], 0), max_rows)) of pix, out and
 *              valid.  Rows at or beyond the device-side count are NOT TOUCHED, so a captured launch stays valid when the count
 *              changes; a negative count is 0.  Both NULL (B must be 1): rows [0, max_rows).
 *   rows       host: how many rows pix, out and valid hold (rows >= max_rows).  A cloud whose rows would leave [0, rows) -- a stale
 *              or corrupt row_begin[b] / row_count[b] -- is skipped WHOLE: nothing of it is read or written, and *err (device int,
 *              caller zeroes, may be NULL) receives PN2_IMAGE_ERR_ROWS.
 *   out        float32 rows of pitch ldo >= 3 floats; EXACTLY three columns per row are written.  The caller may pass a pointer into
 *              a wider row: with out = rows + 4, ldo = 7 the rows x, y, z, i, c0, c1, c2 are painted in place.
 *   valid      uint8 [rows] (1: the point is in the image), may be NULL.
 * THE RULE, per point (x, y):
 *   in the image iff 0 <= y && y < H && 0 <= x && x < W -- the reference's test (:64, whose names x / y are swapped).  It works on
 *   TRUNCATED coordinates: a projected coordinate in (-1, 0) has become 0 and counts as inside.  That quirk is kept.
 *   outside the image, or INT32_MIN: three +0.0 and valid = 0.
 *   NO DEPTH TEST: as in the reference, a point BEHIND the camera that projects into the frame takes that pixel.  The caller
 *   filters first (pn2_scan_filter with the `inview` angles keeps only what the camera sees).
 *   mode RGB: (float)R, (float)G, (float)B; normalised: each divided by 255.0f, one IEEE float32 division.
 *   mode HSV: OpenCV's 8-bit COLOR_BGR2HSV integers as floats, by this rule on the integers r, g, b:
 *     v = max(r, g, b);  d = v - min(r, g, b);  s = (d * sdiv[v] + 2048) >> 12;
 *     h0 = (v == r) ? g - b : (v == g) ? b - r + 2 d : r - g + 4 d   (tested in that order);
 *     h = (h0 * hdiv[d] + 2048) >> 12 (an arithmetic shift), plus 180 if negative;
 *     sdiv[i] = rint(255 * 4096 / i), hdiv[i] = rint(180 * 4096 / (6 i)), round-half-even in fp64, both 0 at i = 0.
 *     The output is (h, s, v): h in 0 .. 179, s and v in 0 .. 255.
 *   HSV normalised: h / 180.0f, s / 255.0f, v / 255.0f as float32 divisions (:68-69, numpy's in-place float32 `/=`): true
 *   divisions, not reciprocal multiplies.
 *   THE HSV RULE IS WRITTEN FROM MEMORY OF OPENCV'S SCALAR CODE AND IS UNVERIFIED AGAINST OPENCV, which was not available where this
 *   was written.  It was checked against the real-valued definition over all 2^24 colours: the hue stays within 0.640 of
 *   30 * sector (circular distance), the saturation within 0.522 of 255 d / v (tests/test_image_sample_cpu.py).
 * PN2_EINVAL without a launch for a null pix / image / out, B < 1 or B > 65535, H or W < 1, H * W * 3 >= 2^31, ldo < 3, an
 * unknown channel_order / mode / normalize, max_rows < 0 or >= 2^31, exactly one of row_begin / row_count NULL, both NULL with
 * B != 1, a pix that is not 8-byte aligned, rows < max_rows.  max_rows == 0 launches nothing. */
#define PN2_CHANNELS_RGB 0
#define PN2_CHANNELS_BGR 1
#define PN2_IMAGE_RGB 0
#define PN2_IMAGE_HSV 1
#define PN2_IMAGE_ERR_ROWS 1
int pn2_sample_image(const int32_t *pix, const uint8_t *image, int B, int H, int W, int channel_order, int mode, int normalize,
                     const int64_t *row_begin, const int64_t *row_count, int64_t max_rows, int64_t rows, float *out, int ldo,
                     uint8_t *valid, int *err, pn2_stream_t stream);
/* pn2_hsv_to_rgb is the way back, for looking at a prediction (the step the reference has commented out at :66-67).  hsv: N float32
 * rows of pitch ld >= 3, three normalised columns (h in units of 180, s and v in units of 255: what pn2_sample_image writes in mode
 * HSV, normalised); out uint8 [N, 3] in the given channel order.  THIS IS THIS PACKAGE'S OWN DEFINITION: OpenCV's HSV2RGB is
 * float-based and is not claimed bit for bit.  In fp64 on the float32 inputs, every operation rounded separately (no fused
 * multiply-add):
 *   s, v clamped to [0, 1];  h6 = (h - floor(h)) * 6;  k = min((int)h6, 5);  f = h6 - k;
 *   p = v * (1 - s),  q = v * (1 - s * f),  t = v * (1 - s * (1 - f));
 *   (r, g, b) = (v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q) for k = 0 .. 5;
 *   each channel is rint(255 * c), round-half-even.
 * A NaN input (or an infinite h, whose fraction is NaN) gives a black pixel.  PN2_EINVAL for ld < 3, N < 0, an unknown
 * channel_order, a null pointer with N > 0. */
int pn2_hsv_to_rgb(const float *hsv, int ld, int64_t N, int channel_order, uint8_t *out, pn2_stream_t stream);

/* ---- panoptic quality: PQ / SQ / RQ counts of instance labels (csrc/panoptic.hip), added within ABI 15 (additive) ---------------------
 * Scores what pn2_voxel_components-style instance ids are worth against a ground truth: per class the matched segments (tp), the
 * unmatched predicted and ground-truth segments (fp, fn) and the sum of the matches' IoU.  THE RULE IS WRITTEN FROM MEMORY OF THE
 * SEMANTICKITTI API'S PanopticEval (addBatchPanoptic, getPQ) AND IS UNVERIFIED AGAINST THE API, which was not available where this was
 * written.  tests/panoptic_ref.py states it in numpy, np.unique per class and side, as the API writes it.
 * Inputs, B clouds in pn2_scan_filter's conventions (device-side row_begin / row_count int64[B], a host bound max_rows; every count is
 * read on the device and clamped to [0, max_rows], rows at or beyond a count are never read, so a captured call stays valid when the
 * counts change):
 *   pred_sem, pred_inst, gt_sem, gt_inst   int32[rows] each; cloud b is rows [row_begin[b], row_begin[b] + row_count[b]);
 *   rows        host: how many rows the four arrays hold (rows >= max_rows).  A cloud whose rows would leave [0, rows) is skipped WHOLE
 *               (nothing of it is read, it adds nothing) and sets PN2_PANOPTIC_ERR_ROWS;
 *   C           classes;   include  int32[C] (device): non-zero = the class is evaluated;
 *   things      int32[C] (device) or NULL.  Where it is given and zero, the instance id of that class counts as 0 on BOTH sides (applied
 *               before rule 5's sign test): one segment per stuff class, what the API's driver script does before it calls the evaluator;
 *   min_points  int32 >= 0 (the API uses 30).
 * Which rows take part:
 *    1. a row takes part iff 0 <= gt_sem < C and include[gt_sem] != 0.  Any other row is dropped from BOTH sides: the API's removal of
 *       ignored ground-truth rows, which shrinks the predicted segments too;
 *    2. a gt_sem outside [0, C) also sets PN2_PANOPTIC_ERR_CLASS.
 * Segments:
 *    3. a participating row belongs to the ground-truth segment (cloud, gt_sem, gt_inst) if gt_inst >= 0;
 *    4. and to the predicted segment (cloud, pred_sem, pred_inst) if pred_inst >= 0, 0 <= pred_sem < C and include[pred_sem] != 0;
 *    5. a negative id: the row has no segment on that side (the API adds 1 and masks out 0);
 *    6. the same id under two classes is two segments; clouds never share segments;
 *    7. a segment's area is its row count.
 * Matching:
 *    8. the intersection of a ground-truth and a predicted segment of the SAME class in the same cloud is the number of rows in both;
 *       union = area_gt + area_pred - inter;
 *    9. the pair is a match iff 2 * inter > union, in integers (= the API's inter / union > 0.5 in fp64 for every union < 2^31);
 *   10. a segment has at most one match (two disjoint overlaps cannot both exceed half of it).
 * Counts, per class:  11. tp = matches;  12. fn = ground-truth segments with area >= min_points and no match;  13. fp = predicted
 *   segments with area >= min_points and no match.
 * IoU sum, per class:
 *   14. for each match q = double(inter) / double(union), ONE IEEE fp64 division: the API's iou, bit for bit;
 *   15. t = q * 2^53 is an exact integer in (2^52, 2^53];
 *   16. the table accumulates iou_hi += t >> 32 and iou_lo += t & 0xFFFFFFFF as int64;
 *   17. the class's IoU sum is the integer S = iou_hi * 2^32 + iou_lo over 2^53, taken on the host as one correctly rounded division.
 * A stated deviation: the API adds the q in fp64, scan by scan; here the sum is exact and rounded once.  The two differ by at most
 *   n_tp * 2^-52 * sum (all terms are positive; each of at most n_tp additions errs by at most 2^-53 of a partial sum that is at most
 *   the total; the factor 2 covers second-order terms).
 * The scores are the host's (fp64, the API's eps = 1e-15): sq = iou / max(tp, eps), rq = tp / max(tp + 0.5 fp + 0.5 fn, eps),
 *   pq = sq * rq, means over the included classes (pointnet12_amd/metrics.py: panoptic_scores).
 * table (int64, 8-byte aligned): [C, 5] with table_stride == 0 (pooled over the clouds), or cloud b's [C, 5] at table + b * table_stride
 *   (table_stride >= 5 * C); columns tp, fp, fn, iou_hi, iou_lo.  The call ADDS into it; the caller zeroes it: an evaluation pass
 *   accumulates on the device and reads back once.  Rows of excluded classes stay as they were.
 * Four plain launches on the caller's stream sized by max_rows; no host synchronisation, no allocation, no thread waits for another
 * thread's write.  Everything that crosses threads is an integer atomic (compare-and-swap, add): the table is the same from run to
 * run, byte for byte, whatever the order of the rows.
 * err (device int, caller zeroes, may be NULL) receives bits disjoint from every other PN2_*_ERR_* bit:
 *   PN2_PANOPTIC_ERR_CLASS  a gt_sem outside [0, C): the row is dropped;
 *   PN2_PANOPTIC_ERR_ROWS   a cloud whose row_begin / row_count leaves the buffers: skipped whole.
 * workspace: pn2_panoptic_workspace_bytes(B, max_rows) bytes of device memory, 16-byte aligned; it may hold anything on entry (per
 * cloud three tables of the power of two >= 2 * max_rows slots of 16 bytes: ground-truth segments, predicted segments, pairs).
 * PN2_EINVAL without a launch, no output touched: a null required pointer (all but things and err), C < 1, B < 1 or B > 65535,
 * max_rows < 0 or > PN2_VOXEL_MAX_ROWS, rows < max_rows, min_points < 0, a table_stride in (0, 5 * C), a pointer that is not 4-byte
 * (row_begin / row_count / table: 8-byte, workspace: 16-byte) aligned; pn2_panoptic_workspace_bytes returns PN2_EINVAL for such
 * B / max_rows.  Out of scope: PQ-dagger, the API's semantic-IoU half (pn2_seg_confusion serves it), tracking metrics, a matching
 * threshold other than 0.5, more than 2^31 - 1 ids or classes. */
#define PN2_PANOPTIC_ERR_CLASS 256
#define PN2_PANOPTIC_ERR_ROWS 512
int64_t pn2_panoptic_workspace_bytes(int B, int64_t max_rows);
int pn2_panoptic_count(const int32_t *pred_sem, const int32_t *pred_inst, const int32_t *gt_sem, const int32_t *gt_inst,
                       const int64_t *row_begin, const int64_t *row_count, int B, int64_t max_rows, int64_t rows, int C,
                       const int32_t *include, const int32_t *things, int min_points, int64_t *table, int64_t table_stride, int *err,
                       void *workspace, pn2_stream_t stream);

/* ---- Lovasz-Softmax loss: the surrogate of mean IoU (csrc/lovasz.hip), added within ABI 15 (additive) ---------------------------------
 * Berman, Triki, Blaschko, "The Lovasz-Softmax loss", CVPR 2018.  The reference repository has no such criterion.  THE RULE IS WRITTEN
 * FROM THE PAPER AND FROM MEMORY OF THE AUTHORS' PUBLISHED lovasz_softmax_flat / lovasz_grad AND IS UNVERIFIED AGAINST THAT CODE, which
 * was not available where this was written.  tests/lovasz_ref.py states it in numpy; tests/test_lovasz_cpu.py holds it to an fp64 torch
 * evaluation of the cumulative-sum formulation.
 * Inputs: x float32, R rows of C <= 64 classes in pn2_cross_entropy_*'s two layouts (inner == 0: x[r * ld + c], ld >= C; inner > 0:
 *   x[(r / inner) * C * inner + c * inner + r % inner]); target int64[R]; images >= 1 divides R: image b is rows [b * R / images,
 *   (b + 1) * R / images) (with inner > 0 and images > 1, inner == R / images).
 * Probabilities: from_logits != 0: p = softmax(x_r) exactly as pn2_cross_entropy_bwd recomputes it, expf((x - max) - logsum), logsum =
 *   logf of the four-way interleaved sum of expf(x - max); log-probabilities are therefore a valid input.  from_logits == 0: p = x.
 * Which rows take part: a row takes part iff target != ignore_index and 0 <= target < C; any other row takes no part, as if it had been
 *   compacted away; an out-of-range target that is not ignore_index also turns the loss NaN (the contract of pn2_nll_loss_*).
 * Segments: one per (image, class).  Segment (b, c) is counted iff (class_mask == NULL or class_mask[c] != 0) and (present_only == 0 or
 *   the segment has at least one foreground row).
 * Per segment, over its participating rows:
 *    1. fg = [target == c];
 *    2. e = fl32(|fg - p|), one float32 subtraction;
 *    3. the rows are ordered by e descending, NaN the largest (every NaN equal), as torch.sort orders them;
 *    4. EQUAL ERRORS COME IN ASCENDING ROW NUMBER (a stable sort; the authors' torch.sort leaves ties undefined);
 *    5. with k the 1-based rank, F_k the foreground rows among the first k and G the segment's foreground count, all integers:
 *         J_k = 1.0 - double(G - F_k) / double(G + k - F_k),  J_0 = 0,  c_k = J_k - J_{k-1}  in fp64
 *       (bit for bit the authors' cumulative-sum form; c_k >= 0 and sum_k c_k <= 1);
 *    6. the segment's loss is l = sum_k double(e_(k)) * c_k.
 * Reduction: per image the mean of l over its counted segments (0 when none is counted), then the mean over ALL images.
 * Gradients: dp[r, c] = float32((w * c_rank(r, c)) * sgn(p - fg)), w = 1.0 / (double(counted segments of the image) * double(images));
 *   sgn(d) = (0 < d) - (d < 0): sgn(0) = 0 as torch.abs, and 0 for NaN; dp is 0 for rows and segments that take no part.
 *   pn2_lovasz_bwd: dx[r, c] = g * (p_c * (dp_c - sum_j p_j * dp_j)) with from_logits (the sum in float32 in class order, p recomputed
 *   as above), g * dp[r, c] otherwise; g = *grad_out is read on the device; dx is written in x's layout, pad columns are never touched.
 * Outputs of pn2_lovasz_fwd: dp float[R, C] (dense); prob float[R, C] or NULL: the probabilities the forward used; loss: one float
 *   (float32 of the fp64 mean: tile partials of 1024 elements, a segment's tiles, the classes and the images each summed in a fixed order).
 * NaN, +inf and e > 1 are ordered per the rule (the sort takes all 32 key bits: four passes of 8), nothing is refused for its values.
 * The forward is 17 plain launches on the caller's stream (keys; 4 x histogram / scan / scatter; foreground count / scan; finalise;
 * reduce); no host synchronisation, no allocation, no workgroup waits on another, positions come from prefix sums of integer counts:
 * the outputs are byte-identical from run to run.  pn2_lovasz_tile_rows() is the tile (elements of a segment per workgroup).
 * workspace: pn2_lovasz_workspace_bytes(R, C, images) bytes of device memory, 16-byte aligned; it may hold anything on entry.  Two
 *   key and two payload buffers of images * C * (R / images) words dominate it: 16 bytes per (row, class) plus 1 KiB of digit counts per
 *   (segment, tile) -- 39 MB of buffers at 16 x 8 000 x 19, 243 MB at 16 x 50 000 x 19.
 * PN2_EINVAL without a launch, no output touched: a null required pointer (all but class_mask and prob), R < 1, C < 1 or C > 64,
 *   images < 1 or not a divisor of R, R / images >= 2^30, R * C >= 2^36, ld < C with inner == 0, inner < 0 or not a divisor of R,
 *   inner > 0 and images > 1 with inner != R / images, a workspace that is not 16-byte aligned;  pn2_lovasz_workspace_bytes returns
 *   PN2_EINVAL for such R / C / images.  Out of scope: the binary hinge, class weights, soft targets, fp16 / bf16 inputs. */
int pn2_lovasz_tile_rows(void);
int64_t pn2_lovasz_workspace_bytes(int64_t R, int C, int images);
int pn2_lovasz_fwd(const float *x, int ld, int64_t inner, const int64_t *target, int64_t R, int C, int images, int64_t ignore_index,
                   int from_logits, const int32_t *class_mask, int present_only, void *workspace, float *dp, float *prob, float *loss,
                   pn2_stream_t stream);
int pn2_lovasz_bwd(const float *x, int ld, int64_t inner, const float *dp, int64_t R, int C, int from_logits, const float *grad_out,
                   float *dx, pn2_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PN2_H */
