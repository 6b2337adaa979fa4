// Host side shared by the three shared-MLP units (mlp.hip: streamed weights, mlp_res.hip: weights in LDS, mlp_wide.hip: weights
// in registers): the upstream-gradient operand, the one declaration of every function that crosses the units, small helpers.
#pragma once
#include "mlp_loaders.h"
#include <algorithm>

inline int round4(int x) { return (x + 3) & ~3; }
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// The kernels that address with 32-bit element offsets: P rows of the widest of these pitches stay below 2^32 elements.
template <class... Ld>
inline bool fits_u32_offsets(int64_t P, Ld... ld) { return P * std::max({(int64_t)ld...}) < (1LL << 32); }

// "This layer's output gradient" as every backward entry point of include/pn2.h takes it: dense (dZ [P, ldz]) or implied by the
// max-pool (dZp, arg [P / Kpool, ldo]), with the layer's pre-BN output Y and the BatchNorm-backward coefficients that turn the
// pair into dY.  (Outside the anonymous namespace like LazyCoef: it crosses the units as an argument.)
struct UpGrad {
    const float *dZ; int ldz;
    const float *dZp; int ldo; const int32_t *arg; int Kpool;
    const float *Y; int ldy; const float *coef;
    LazyCoef lc;                                    // `coef` is filled by the prologue of the FIRST launch that reads it
    bool dense() const { return dZ != nullptr; }
    // what every entry point requires for a layer of C_out channels: dense, or pooled with a positive group size; float4 rows
    bool valid(int C_out, bool dz_pitch = true) const {
        const int c4 = round4(C_out);
        return Y && coef && (dZ || (dZp && arg && Kpool > 0)) && ldy % 4 == 0 && ldy >= c4 &&
               (!dz_pitch || (dZ ? ldz % 4 == 0 && ldz >= c4 : ldo % 4 == 0 && ldo >= c4));
    }
    UpGrad without_lazy() const { UpGrad o = *this; o.lc = LazyCoef{}; return o; }
    // The rows behind the first `rows`, which an earlier launch covered (whole pooling groups: the tile heights divide Kpool or
    // are multiples of it) -- and with them the lazy record: that launch filled the coefficient block.
    UpGrad advanced(int64_t rows) const {
        UpGrad o = without_lazy();
        if (dZ) o.dZ += rows * ldz;
        else { o.dZp += (rows / Kpool) * ldo; o.arg += (rows / Kpool) * ldo; }
        o.Y += rows * ldy;
        return o;
    }
};

// Defined in one unit, called from another.  rows_done: the leading rows a pn2_wide_* launch covered (whole tiles).
int pn2_fwd_res(const float *X, int ldx, const float *in_affine, const float *W, int ldw, const float *bias, float *Y, int ldy,
                int64_t P, int K, int N, double *stats, LazyBn lz, hipStream_t s);                                  // mlp_res.hip
int pn2_wide_fwd(const float *X, int ldx, const float *in_affine, const float *W, int ldw, const float *bias, float *Y, int ldy,
                 int64_t P, int K, int N, double *stats, LazyBn lz, hipStream_t s, int64_t *rows_done, int Kpool = 0,
                 const float *pool_gamma = nullptr, float *pool_ws = nullptr);                                      // mlp_wide.hip
int pn2_wide_dgrad(const UpGrad &up, const float *W, int ldw, const float *prev_Y, int ld_prev, const float *prev_affine, float *dXout,
                   int ldxo, double *prev_red, int64_t P, int K, int N, hipStream_t s, int64_t *rows_done);           // mlp_wide.hip
int pn2_wide_wgrad(const UpGrad &up, const float *X, int ldx, const float *x_affine, float *dW, int lddw, float *dbias, int64_t P,
                   int M, int N, hipStream_t s, float *workspace = nullptr);                                        // mlp_wide.hip
int64_t pn2_wide_wgrad_workspace_bytes(int64_t P, int M, int N, int pooled);                                        // mlp_wide.hip
// pn2_conv1x1_dgrad / pn2_conv1x1_wgrad_ws behind the ABI (mlp.hip): every check of theirs but the lazy record's
struct PairJob;     // (mlp.hip: the weight-gradient half pn2_conv1x1_bwd_pair wants to ride in the data gradient's launch)
int pn2_dgrad_up(UpGrad up, const float *W, int ldw, const float *prev_Y, int ld_prev, const float *prev_affine, float *dXout, int ldxo,
                 double *prev_red, int64_t P, int K, int N, hipStream_t s, PairJob *job = nullptr);
int pn2_wgrad_up(const UpGrad &up, const float *X, int ldx, const float *x_affine, float *dW, int lddw, float *dbias, int64_t P, int M,
                 int N, float *workspace, hipStream_t s);

namespace {

template <class A, class B> struct same { static constexpr bool v = false; };
template <class A> struct same<A, A> { static constexpr bool v = true; };

// The conversions of an UpGrad to what the kernels take.  (Free functions: the loader and argument types are per unit.)
// f(loader of dY, coefficient rows of pitch ldc): the dense / pooled choice, made once per entry point
template <class F>
int with_dy(const UpGrad &up, int ldc, F &&f) {
    if (up.dense()) return f(LoadDyDense{up.dZ, up.ldz, up.Y, up.ldy, up.coef, ldc, zero_page_dev(), up.lc});
    return f(LoadDyPooled{up.dZp, up.ldo, up.arg, up.Kpool, up.Y, up.ldy, up.coef, ldc, zero_page_dev(), pow2_shift(up.Kpool), up.lc});
}
template <class ResDy>                              // mlp_res.hip's kernel argument (Y and a dense dZ share one pitch there)
ResDy res_dy(const UpGrad &up) { return ResDy{up.dZ, up.dZp, up.arg, up.ldo, up.dense() ? 0 : pow2_shift(up.Kpool), up.Y, up.ldy, up.coef, up.lc}; }
template <class Args>                               // the dZ fields of mlp_wide.hip's RegwArgs / WgradArgs (group size: a template parameter)
void fill_dz(Args &g, const UpGrad &up) { g.dZ = up.dZ; g.ldz = up.ldz; g.dZp = up.dZp; g.arg = up.arg; g.ldo = up.ldo; }

}  // namespace
