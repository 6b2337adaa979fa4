"""Operands, fp64 statements, a-priori bounds, case tables and float32 emulations of the PointNet v1 entry points
(csrc/pointnet_v1.hip, csrc/pointnet_dense.hip and the K-concatenated GEMMs of csrc/mlp.hip): pn2_point_transform / _bwd,
pn2_bn_max, pn2_pool_bwd_reduce_noact, pn2_conv1x1_fwd_gbias, pn2_group_colsum, pn2_bn_bwd_reduce_noact_dense,
pn2_conv1x1_fwd_multi / _wgrad_multi / _dgrad_multi and the two workspace formulas.  A test helper in the style of
tests/bn_pool_ref.py, written from the formulas of include/pn2.h, for clarity, not speed.  Everything is numpy; every operand
set is drawn on the CPU from a seed, so tests/test_pointnet_v1_kernels_ref_cpu.py (no GPU) and
tests/test_pointnet_v1_edges_gpu.py see the SAME numbers.

BUFFERS.  Every operand is a [rows, pitch] float32 array.  An input holds its values in the leading C columns, zeros in
[C, round4(C)) where the contract asks for zero pad columns, and NaN from round4(C) to the pitch: a kernel that reads one
column too many turns a result into NaN.  (dOut of pn2_pool_bwd_reduce_noact and gbias of pn2_conv1x1_fwd_gbias have no pad
contract -- "any pitch >= C": they hold NaN from column C on.)  An output starts as SENTINEL bits (a NaN no kernel produces)
in every element, its rows followed by GUARD rows: whatever the contract does not name must come back as SENTINEL.  A workspace
is filled with NaN ("contents irrelevant") and followed by a SENTINEL guard.

STATEMENTS.  One function per entry point with the entry point's name and the pitches in its argument list, numpy fp64.

BOUNDS -- counted, none fitted to a result.  u = 2^-24.
  ``bound(n, A, k)`` = (n + 2 + k) u A: an fp32 fma chain of length n, or an fp32 sum of n terms in any order, on terms that
      carry k roundings of their own, A = the sum of the terms' absolute values computed from the operands (Higham 4.2: the
      factor is n - 1 + k to first order; + 3 covers the denominator for n < 1e5 and the fp64 rounding of A).
  transform / dX: n = round4(k) (the pad quads are walked too: zeros);  dT: n = N, whatever the lane and slab tree (adding a
      zero is exact, so idle lanes and empty slabs add nothing);  fwd_gbias: the K products, the bias and the per-cloud term,
      n = K + 2;  the multi-source forward the same with K = sum K_i, its BatchNorm sources entering as the fp64 value of
      fma(fl(x - mean), scale, beta) (k = 1: its rounding to float32);  dgrad: n = M on dY of three roundings;  wgrad: n = P on
      dY * act (k = 4), dbias n = P, k = 3;  group_colsum: n = rows_per_group, k = 3.
  fp64 reductions (red, stats): (n + 8) 2^-53 A for the fp64 additions plus the float32 roundings of a term: none for sum dZ
      and for sum y / sum y^2 of pn2_conv1x1_fwd_gbias (taken in fp64 on the float32 y the kernel stored: compared against the
      stored Y), 3.01 u for dz * ((y - mean) * invstd).  The multi-source forward sums a tile's rows in fp32 first: bound(P, A)
      and bound(P, A, 1).
  Bit comparisons where the contract fixes the arithmetic: bn_max out / arg (lattice operands, bn_pool_ref: fma exact), dZp
      (a copy), dZ of the dense reduction (dyadic operands: the one addition is exact) and its red0, written zeros, SENTINELs,
      and "two launches identical" (dT, the column sums).
  Against the older tests: tests/test_pointnet_v1_gpu.py holds these kernels to 3e-6 (transform, dX, Y) and 1e-5 (dT, column
  sums) of the tensor's LARGEST entry.  The bounds here are per element and relative to the sum of |terms| of that element, and
  at the existing shapes they come out LOOSER than those figures: on standard normal operands sum |x t| is about 0.64 n times a
  term and the largest entry about 4 sqrt(n) terms, so the transform at k = 128 is allowed 130 u * 0.64 * 128 / (4 sqrt(128))
  = 1.4e-5 of the largest entry against 3e-6, and dT at N = 25 000 some 4e-2 against 1e-5 -- a worst-case bound grows like n
  where the error of n independent roundings grows like sqrt(n).  They are tight where it matters here: at the small n of these
  tables one dropped or misplaced term leaves its bound on every case (the mutants of the CPU test).  The older tests keep their
  tolerances.

EMULATIONS.  ``emulate_*`` follow the kernels' arithmetic in float32 -- the summation order too where the contract fixes it
(the lanes and slabs of dT and of the column sums, the row lanes of bn_max and their fold) -- and take a ``mutant``:
  "slab_last_row"  the last row of every 256-row slab (or row range) is skipped
  "last_slab"      the second launch adds all slabs but the last
  "gbias_late"     the per-cloud term's group boundary one row late: gbias[(p - 1) / rows_per_group]
  "if_advance"     (g, k) of the dense reduction advanced with `if (k >= K)` instead of `while`
  "last_k"         a row lane keeps the LAST row attaining its maximum (>=)
  "no_smaller_k"   the lane fold without "equal and smaller k"
  "idle_lane"      the lane fold takes the smaller k whatever the value: an idle lane's (-inf, 0) beats every real row
  "t_untransposed" the dX form stages the quad rows / columns of T_b that hold pad columns untransposed
  "dt_store_past"  the dT slab store without `i < k`: rows [k, round4(k)) are written behind the slab's k * k elements
  "pitch_for_width" pn2_pool_bwd_reduce_noact reads dOut at pitch ldo instead of ld_dout
  "replica_missing" one replica of a `red` / `stats` block is not summed
``check_*`` hold what the GPU test asserts (bounds, bit comparisons, sentinels) and return the list of violations: empty for the
emulation and for the kernels, non-empty for a mutant on every case it changes anything on.
"""
import numpy as np

from bn_pool_ref import U32, U64, fma32
from mlp_ref import SENTINEL, STAT_REPLICAS, round4

f32, f64, i32 = np.float32, np.float64, np.int32
SLAB = 256                           # kTfRows: rows of one dT / column-sum slab
MAX_K = 128                          # kTfMaxK
MULTI_MAX = 8                        # PN2_MULTI_MAX
NOMINAL_CUS = 256                    # an MI355X; the row ranges of the two row-walking kernels depend on pn2_num_cus()
GUARD = 8                            # guard rows behind every output
MUTANTS = ("slab_last_row", "last_slab", "gbias_late", "if_advance", "last_k", "no_smaller_k", "idle_lane", "t_untransposed",
           "dt_store_past", "pitch_for_width", "replica_missing")


def cdiv(a, b):
    return -(-a // b)


def bound(n, A, k=0):
    return (n + 2 + k) * U32 * A


def padded(values, ld, pad_to=None, tail=np.nan):
    """float32 [P, ld]: `values` [P, C], zeros up to pad_to (default round4(C)), `tail` behind."""
    P, C = values.shape
    t = np.full((P, ld), tail, f32)
    t[:, :C] = values
    t[:, C:min(ld, round4(C) if pad_to is None else pad_to)] = 0.0
    return t


def sentinel(rows, ld):
    """float32 [rows + GUARD, ld] of SENTINEL bits."""
    return np.full((rows + GUARD, ld), SENTINEL, i32).view(f32)


def is_sentinel(a):
    return np.ascontiguousarray(a).view(i32) == SENTINEL


def block(*rows4):
    """float32 [4 * round4(C)] block (affine: mean | scale | beta | invstd; coef: c0 | q1 | q0 | mean), pad entries zero."""
    C = len(rows4[0])
    b = np.zeros((4, round4(C)), f32)
    for i, r in enumerate(rows4):
        b[i, :C] = r
    return b.reshape(-1)


def red_total(red, C):
    return np.asarray(red, f64).reshape(STAT_REPLICAS, 2, C).sum(0)


# ================================================================================================ workspace formulas

def point_transform_workspace_bytes(B, N, k):
    return 0 if B <= 0 or N <= 0 or k <= 0 or k > MAX_K else B * cdiv(N, SLAB) * k * k * 4


def group_colsum_workspace_bytes(P, rpg, C):
    return 0 if P <= 0 or rpg <= 0 or C <= 0 or P % rpg else (P // rpg) * cdiv(rpg, SLAB) * round4(C) * 4


# ================================================================================================ fp64 statements

def _c(buf, P, ld, C, dt=f64):
    return np.asarray(buf).reshape(-1)[:P * ld].reshape(P, ld)[:, :C].astype(dt)


def point_transform(X, ldx, T, B, N, k):
    """out[b N + n, j] = sum_i X[b N + n, i] T[b, i, j]; returns (out [B N, k], bound)."""
    x, t = _c(X, B * N, ldx, k).reshape(B, N, k), T.astype(f64)
    out, A = np.einsum("bni,bij->bnj", x, t), np.einsum("bni,bij->bnj", np.abs(x), np.abs(t))
    return out.reshape(B * N, k), bound(round4(k), A).reshape(B * N, k)


def point_transform_bwd(D, ldd, X, ldx, T, B, N, k):
    """dX = dOut T_b^T, dT_b = sum_n X_n^T dOut_n; returns (dX, bound, dT, bound)."""
    d, x, t = _c(D, B * N, ldd, k).reshape(B, N, k), _c(X, B * N, ldx, k).reshape(B, N, k), T.astype(f64)
    dX, AX = np.einsum("bnj,bij->bni", d, t), np.einsum("bnj,bij->bni", np.abs(d), np.abs(t))
    dT, AT = np.einsum("bni,bnj->bij", x, d), np.einsum("bni,bnj->bij", np.abs(x), np.abs(d))
    return dX.reshape(B * N, k), bound(round4(k), AX).reshape(B * N, k), dT, bound(N, AT)


def bn_max(Y, ldy, aff, G, K, C):
    """out[g, c] = max_k fma(fl(y - mean), scale, beta), arg = the first k attaining it (numpy's argmax)."""
    a = aff.reshape(4, -1)
    y = _c(Y, G * K, ldy, C, f32).reshape(G, K, C)
    z = (y - a[0, :C]).astype(f64) * a[1, :C].astype(f64) + a[2, :C].astype(f64)
    return z.max(1), z.argmax(1).astype(i32)


def pool_bwd_reduce_noact(dOut, ld_dout, arg, ldo, Y, ldy, aff, G, K, C):
    """dZp = dOut; red0 = sum_g dOut, red1 = sum_g dOut yhat(Y[g K + arg]); returns (dZp f32, red0, b0, red1, b1)."""
    a = aff.reshape(4, -1).astype(f64)
    flat = np.asarray(dOut).reshape(-1)
    d32 = flat[(np.arange(G)[:, None] * ld_dout + np.arange(C)[None, :])]
    d = d32.astype(f64)
    ag = _c(arg, G, ldo, C, np.int64)
    y = _c(Y, G * K, ldy, C).reshape(G, K, C)
    ysel = np.take_along_axis(y, ag[:, None, :], 1)[:, 0]
    xh = (ysel - a[0, :C]) * a[3, :C]
    A0, A1 = np.abs(d).sum(0), np.abs(d * xh).sum(0)
    b0 = (G + 8) * U64 * A0
    return d32.astype(f32), d.sum(0), b0, (d * xh).sum(0), 3.01 * U32 * A1 + (G + 8) * U64 * A1 + b0


def conv1x1_fwd_gbias(X, ldx, W, bias, gbias, ldg, rpg, P, K, N):
    """Y[p, c] = (X W^T)[p, c] + bias[c] + gbias[p / rows_per_group, c] (W the [N, K] window); returns (Y, bound)."""
    x, w = _c(X, P, ldx, K), W.astype(f64)
    g = _c(gbias, P // rpg, ldg, N)
    gp = np.repeat(g, rpg, 0)
    y = x @ w.T + bias.astype(f64) + gp
    A = np.abs(x) @ np.abs(w).T + np.abs(bias.astype(f64)) + np.abs(gp)
    return y, bound(K + 2, A)


def dy_of(dZ, ldz, Y, ldy, coef, P, C):
    c = coef.reshape(4, -1).astype(f64)[:, :C]
    t = (c[0] * _c(dZ, P, ldz, C), c[1] * (_c(Y, P, ldy, C) - c[3]), np.broadcast_to(c[2], (P, C)))
    return t[0] + t[1] + t[2], np.abs(t[0]) + np.abs(t[1]) + np.abs(t[2])


def group_colsum(dZ, ldz, Y, ldy, coef, P, rpg, C):
    """s[g, c] = sum over the rows of group g of dY = c0 dZ + q1 (y - mean) + q0; returns (s, bound)."""
    dY, A = dy_of(dZ, ldz, Y, ldy, coef, P, C)
    G = P // rpg
    return dY.reshape(G, rpg, C).sum(1), bound(rpg, A.reshape(G, rpg, C).sum(1), 3)


def bn_bwd_reduce_noact_dense(dDense, ldd, dPool, ldp, arg, lda, Y, ldy, aff, G, K, C):
    """dZ = dDense + (k == arg) dPool; red0 = sum dZ, red1 = sum dZ yhat; returns (dZ fp64, red0, b0, red1, b1)."""
    P = G * K
    a = aff.reshape(4, -1).astype(f64)
    hit = np.arange(K)[None, :, None] == _c(arg, G, lda, C, np.int64)[:, None, :]
    dZ = (_c(dDense, P, ldd, C).reshape(G, K, C) + np.where(hit, _c(dPool, G, ldp, C)[:, None, :], 0.0)).reshape(P, C)
    xh = (_c(Y, P, ldy, C) - a[0, :C]) * a[3, :C]
    A0, A1 = np.abs(dZ).sum(0), np.abs(dZ * xh).sum(0)
    b0 = (P + 8) * U64 * A0
    return dZ, dZ.sum(0), b0, (dZ * xh).sum(0), 3.01 * U32 * A1 + (P + 8) * U64 * A1 + b0


def multi_operand(srcs, P):
    """The virtual concatenation in fp64: srcs [(X, ldx, K, affine block or None, relu)]; a BatchNorm source enters as
    fma(fl(x - mean), scale, beta) (the subtraction in float32, as the loader does it), then the ReLU."""
    out = []
    for X, ldx, K, aff, relu in srcs:
        x = _c(X, P, ldx, K, f32)
        if aff is None:
            out.append(x.astype(f64))
            continue
        a = aff.reshape(4, -1)
        v = (x - a[0, :K]).astype(f64) * a[1, :K].astype(f64) + a[2, :K].astype(f64)
        out.append(np.maximum(v, 0.0) if relu else v)
    return np.concatenate(out, 1)


def conv1x1_fwd_multi(srcs, W, bias, gbias, ldg, rpg, P, N):
    """Y = A W^T + bias (+ gbias per group); returns (Y, bound)."""
    A_, w = multi_operand(srcs, P), W.astype(f64)
    y = A_ @ w.T + bias.astype(f64)
    A = np.abs(A_) @ np.abs(w).T + np.abs(bias.astype(f64))
    if gbias is not None:
        gp = np.repeat(_c(gbias, P // rpg, ldg, N), rpg, 0)
        y, A = y + gp, A + np.abs(gp)
    return y, bound(A_.shape[1] + 2, A, 1)


def conv1x1_wgrad_multi(dZ, ldz, Y, ldy, coef, srcs, P, M):
    """dW[m, j] = sum_p dY[p, m] A[p, j], dbias[m] = sum_p dY[p, m]; returns (dW, bound, dbias, bound)."""
    dY, AY = dy_of(dZ, ldz, Y, ldy, coef, P, M)
    A_ = multi_operand(srcs, P)
    return dY.T @ A_, bound(P, AY.T @ np.abs(A_), 4), dY.sum(0), bound(P, AY.sum(0), 3)


def conv1x1_dgrad_multi(dZ, ldz, Y, ldy, coef, W, Ks, P, M):
    """dX_i = dY W[:, k_i : k_i + K_i]; returns [(dX_i, bound)]."""
    dY, AY = dy_of(dZ, ldz, Y, ldy, coef, P, M)
    out, k0 = [], 0
    for K in Ks:
        w = W[:, k0:k0 + K].astype(f64)
        out.append((dY @ w, bound(M, AY @ np.abs(w), 3)))
        k0 += K
    return out


# ================================================================================================ case tables

TRANSFORM_K = (1, 2, 3, 5, 8, 12, 13, 20, 33, 60, 61, 64, 65, 68, 100, 127, 128)
TRANSFORM_N = (1, 3, 255, 256, 257, 600)


def transform_geometry(k):
    """(q, row lanes of the forward, idle threads there, dT blocks, dT row lanes, idle threads there, dT trips)."""
    q = round4(k) // 4
    nblk = q * q
    lanes = 256 // nblk if nblk < 256 else 1
    return q, 256 // q, 256 - (256 // q) * q, nblk, lanes, max(0, 256 - lanes * nblk) if nblk < 256 else 0, cdiv(nblk, 256)


def _k_seam(k):
    q, rp, idle, nblk, lanes, idle_t, trips = transform_geometry(k)
    s = "q=%d" % q
    if idle:
        s += " %d-idle" % idle
    if nblk < 256:
        s += " one-lane" if lanes == 1 else " dT-%d-lanes" % lanes
        if idle_t and lanes <= 3:
            s += " %d-idle" % idle_t
    else:
        s += " %d-blocks" % nblk + (" %d-trips" % trips if trips > 1 else "")
    return s + (" pad" if k % 4 else "")


def transform_cases():
    """[(id, seed, B, N, k)]: every k at N = 257 (a slab of 256 rows and one more), B = 3; every N at k in {5, 33, 64, 68} with
    B alternating 1 / 3.  N seams: 1 and 3 rows (fewer than any lane count), 255 / 256 / 257 around one slab, 600 = three slabs
    with a partial last one."""
    out = [("k=%d %s N=257 B=3" % (k, _k_seam(k)), 2000 + k, 3, 257, k) for k in TRANSFORM_K]
    nseam = {1: "one-row", 3: "rows<lanes", 255: "slab-1", 256: "one-slab", 257: "slab+1", 600: "three-slabs"}
    for k in (5, 33, 64, 68):
        for j, N in enumerate(TRANSFORM_N):
            if N != 257:
                out.append(("k=%d N=%d %s B=%d" % (k, N, nseam[N], (1, 3)[j % 2]), 2200 + 7 * k + j, (1, 3)[j % 2], N, k))
    return out


BN_MAX_C = (1, 3, 4, 5, 16, 17, 20, 63, 64, 65)
BN_MAX_K = (1, 2, 63, 64, 65, 130)


def bn_max_cases():
    """[(id, seed, G, K, C, with_arg)]: C x K with G alternating 1 / 3 (C = 16 | 17: one and two 16-channel workgroups; K = 1, 2,
    63: idle lanes holding (-inf, 0); 64: every lane one row; 65, 130: lanes that visit two and three rows), G = 65539 behind the
    65535 grid rows, and one call without arg."""
    kseam = {1: "63-idle-lanes", 2: "62-idle-lanes", 63: "one-idle-lane", 64: "full-lanes", 65: "lane-revisit", 130: "three-visits"}
    out = []
    for i, C in enumerate(BN_MAX_C):
        for j, K in enumerate(BN_MAX_K):
            G = (1, 3)[(i + j) % 2]
            out.append(("C=%d K=%d %s G=%d" % (C, K, kseam[K], G), 3000 + 10 * i + j, G, K, C, True))
    out.append(("G=65539 grid-stride K=2 C=4", 3200, 65536 + 3, 2, 4, True))
    out.append(("C=5 K=65 G=3 arg=NULL", 3201, 3, 65, 5, False))
    return out


def pool_bwd_cases():
    """[(id, seed, G, K, C, ld_dout, ldy, arg mode)]: C x G; ld_dout in {C, C + 1, round4(C) + 4}, ldy in {round4(C), + 8}, arg from
    the bn_max statement | all 0 | all K - 1.  G = 4, 5 around the four group lanes, G = 4099 a second trip behind 1024 workgroups."""
    out = []
    for i, C in enumerate(BN_MAX_C + (130,)):
        for j, G in enumerate((1, 3, 4, 5, 4099)):
            K = 2 if G == 4099 else (1, 3, 5)[(i + j) % 3]
            ldd = (C, C + 1, round4(C) + 4)[(i + j) % 3]
            ldy = round4(C) + (0, 8)[(i + j // 3) % 2]
            mode = ("bn_max", "zero", "last")[(i + 2 * j) % 3]
            seam = " grid-stride" if G == 4099 else ""
            out.append(("C=%d G=%d%s K=%d ld_dout=%d ldy=%d arg=%s" % (C, G, seam, K, ldd, ldy, mode), 4000 + 10 * i + j, G, K, C, ldd, ldy, mode))
    return out


def gbias_cases():
    """[(id, seed, P, K, N, rpg, stats, ldg)]: output width N x rows_per_group with three groups; K, stats and ldg cycle.
    rows_per_group 1 (a group per row), 3 (five groups inside a 16-row range), 16 (= the range), 17 (a group straddles a
    range's end), 500 (many ranges inside a group); N = 255 / 256 / 257 / 260 around the 256 columns of a workgroup."""
    rseam = {1: "group-per-row", 3: "groups-inside-range", 16: "group=range", 17: "group-straddles-range", 500: "ranges-inside-group"}
    out, n = [], 0
    for i, N in enumerate((1, 5, 64, 255, 256, 257, 260)):
        for j, rpg in enumerate((1, 3, 16, 17, 500)):
            K = (4, 8, 64)[(i + j) % 3]
            stats = (i + j // 2) % 2 == 0
            ldg = N if (i + j) % 2 else round4(N) + 4
            out.append(("N=%d rpg=%d %s K=%d stats=%d ldg=%d" % (N, rpg, rseam[rpg], K, stats, ldg), 5000 + n, 3 * rpg, K, N, rpg, stats, ldg))
            n += 1
    return out


def colsum_cases():
    """[(id, seed, G, rpg, C, lds)]: rows_per_group x C, G alternating 1 / 3, lds in {C, round4(C), round4(C) + 4}."""
    rseam = {1: "one-row", 3: "rows<lanes", 255: "slab-1", 256: "one-slab", 257: "slab+1", 600: "three-slabs"}
    out, n = [], 0
    for i, rpg in enumerate((1, 3, 255, 256, 257, 600)):
        for j, C in enumerate((1, 5, 64, 255, 257)):
            lds = (C, round4(C), round4(C) + 4)[(i + j) % 3]
            out.append(("rpg=%d %s C=%d G=%d lds=%d" % (rpg, rseam[rpg], C, (1, 3)[(i + j) % 2], lds), 6000 + n, (1, 3)[(i + j) % 2], rpg, C, lds))
            n += 1
    return out


def row_range(cus, P, C, floor):
    """Rows per workgroup of the two row-walking launches: cdiv(P, 4 cus / gx) with gx = cdiv(round4(C), 256), at least `floor`."""
    wgs = max(1, cus * 4 // cdiv(round4(C), 256))
    return max(floor, cdiv(P, wgs))


def dense_cases(cus=NOMINAL_CUS):
    """[(id, seed, G, K, C)]: K x C.  G is the smallest count with more than two 64-row ranges and P = G K no multiple of 64
    (K = 64: every P is one; G = 3).  A group straddles a range's end wherever K does not divide 64 (K = 3, 5, 63, 65, 500);
    for K = 1, 2, 64 none can.  K = 1, 2, 3 are the `while` of the incremental (g, k) advance: a thread steps four rows, that is
    four, two, and one or two groups."""
    kseam = {1: "while-advance four-groups-a-step", 2: "while-advance two-groups-a-step", 3: "while-advance straddle", 5: "straddle",
             63: "straddle", 64: "group=range", 65: "straddle", 500: "ranges-inside-group"}
    out, n = [], 0
    for K in (1, 2, 3, 5, 63, 64, 65, 500):
        for C in (1, 5, 36, 255, 256, 257, 260):
            G = 3 if K == 64 else next(g for g in range(1, 200) if g * K > 128 and (g * K) % 64)
            assert row_range(cus, G * K, C, 64) == 64
            out.append(("K=%d %s G=%d C=%d" % (K, kseam[K], G, C), 7000 + n, G, K, C))
            n += 1
    return out


MULTI_TABLE = ((8, 8, "id"), (4, 8, "id"), (12, 12, "bn"), (4, 8, "relu"), (16, 20, "id"), (4, 4, "id"), (8, 16, "relu"), (12, 16, "id"))


def multi_cases():
    """[(id, seed, P, N, mode)]: eight sources (K, pitch, activation) of MULTI_TABLE -- a K = 4 source with ReLU in the middle --
    P in {1, 63, 65, 257} x output width in {1, 13, 50}; mode "rpg1": rows_per_group = 1 with stats, "nog": gbias NULL with stats,
    "one": one group, no stats."""
    out, n = [], 0
    for i, P in enumerate((1, 63, 65, 257)):
        for j, N in enumerate((1, 13, 50)):
            mode = ("rpg1", "nog", "one")[(i + j) % 3]
            out.append(("P=%d N=%d nsrc=8 %s" % (P, N, {"rpg1": "rows_per_group=1", "nog": "gbias=NULL stats", "one": "one-group"}[mode]), 8000 + n, P, N, mode))
            n += 1
    return out


# ================================================================================================ operands

def _lattice_affine(rng, C, seed):
    mean = (rng.integers(-128, 129, C) / 64.0).astype(f32)
    mag = rng.integers(2, 17, C) / 8.0
    kind = (np.arange(C) + seed) % 5
    scale = np.where(kind == 3, 0.0, np.where(kind % 2 == 1, -mag, mag)).astype(f32)
    beta = (rng.integers(-16, 17, C) / 16.0).astype(f32)
    return mean, scale, beta


def operands(seed, kind, **d):
    """Every buffer of one call of `kind`, drawn from `seed` (module docstring: BUFFERS).  Returns a dict."""
    rng = np.random.default_rng(seed)
    nrm = lambda *s: rng.standard_normal(s).astype(f32)
    if kind == "transform":
        B, N, k = d["B"], d["N"], d["k"]
        kp = round4(k)
        o = dict(d, ldx=kp, ldo=kp + 4, ldd=kp + 8, lddx=kp + 12)
        o["X"], o["D"] = padded(nrm(B * N, k), o["ldx"]), padded(nrm(B * N, k), o["ldd"])
        o["T"] = (nrm(B, k, k) / f32(k ** 0.5)).astype(f32)
        return o
    if kind == "bn_max":
        G, K, C = d["G"], d["K"], d["C"]
        mean, scale, beta = _lattice_affine(rng, C, seed)
        Y = (rng.integers(-500, 501, (G, K, C)) / 64.0).astype(f32)
        ext = np.where(scale < 0, -8.0, 8.0).astype(f32)
        # (k, k + 1): neighbouring lanes; (k, k + 64): one lane's two visits, its strict >; (0, K - 1): the ends; (1, 64): the smaller
        # k sits on the LATER lane, the fold's "equal and smaller k"
        pairs = [(k0, k1) for k0, k1 in ((K // 2, K // 2 + 1), (K // 3, K // 3 + 64), (0, K - 1), (1, 64)) if k0 < k1 < K]
        plants = np.full((G, C), -1, i32)                 # index into `pairs`, -1: none
        for g in range(min(G, 8)):                       # planted exact ties of the extreme: the first row of the pair wins
            for c in range(C):
                if pairs and (g * C + c + seed) % 4 != 3:          # (a quarter stay free: their maximum is wherever it falls)
                    plants[g, c] = (g + c + seed) % len(pairs)
                    k0, k1 = pairs[plants[g, c]]
                    Y[g, k0, c] = Y[g, k1, c] = ext[c]
        o = dict(d, ldy=round4(C) + 4, ldo=round4(C) + 8, mean=mean, scale=scale, beta=beta, plants=plants, pairs=pairs)
        o["invstd"] = rng.uniform(0.5, 2.0, C).astype(f32)
        o["Y"], o["aff"] = padded(Y.reshape(G * K, C), o["ldy"]), block(mean, scale, beta, o["invstd"])
        return o
    if kind == "pool_bwd":
        G, K, C = d["G"], d["K"], d["C"]
        o = operands(seed, "bn_max", G=G, K=K, C=C)
        o.update(d)
        o["Y"] = padded(o["Y"][:, :C], d["ldy"])
        if d["mode"] == "bn_max":
            arg = bn_max(o["Y"], d["ldy"], o["aff"], G, K, C)[1]
        else:
            arg = np.full((G, C), 0 if d["mode"] == "zero" else K - 1, i32)
        o["arg"] = np.zeros((G, o["ldo"]), i32)
        o["arg"][:, :C] = arg
        dOut = np.full(G * d["ld_dout"] + 4, np.nan, f32)            # "any pitch >= C": no pad contract, NaN from column C on
        dOut[:G * d["ld_dout"]].reshape(G, d["ld_dout"])[:, :C] = (rng.integers(-1024, 1025, (G, C)) / 256.0).astype(f32)
        o["dOut"] = dOut
        return o
    if kind == "gbias":
        P, K, N, rpg = d["P"], d["K"], d["N"], d["rpg"]
        off = 8
        o = dict(d, ldx=K + 4, ldy=round4(N) + 4, off=off, ldw=off + K + 4)
        o["X"] = padded(nrm(P, K), o["ldx"])
        o["Wfull"] = np.full((N, o["ldw"]), np.nan, f32)
        o["Wfull"][:, off:off + K] = nrm(N, K) / f32(K ** 0.5)
        o["W"] = o["Wfull"][:, off:off + K]
        o["bias"] = nrm(N)
        o["gbias"] = padded(nrm(P // rpg, N), d["ldg"], pad_to=N)
        return o
    if kind == "colsum":
        G, rpg, C = d["G"], d["rpg"], d["C"]
        P = G * rpg
        o = dict(d, P=P, ldz=round4(C) + 4, ldy=round4(C) + 8)
        o["dZ"], o["Y"] = padded(nrm(P, C), o["ldz"]), padded(nrm(P, C), o["ldy"])
        o["coef"] = block(nrm(C) * f32(0.5) + f32(1), nrm(C) * f32(0.05), nrm(C) * f32(0.05), nrm(C) * f32(0.3))
        return o
    if kind == "dense":
        G, K, C = d["G"], d["K"], d["C"]
        P, c4 = G * K, round4(C)
        o = dict(d, P=P, ldd=c4 + 4, ldp=c4 + 8, lda=c4 + 12, ldy=c4 + 16, ldz=c4)
        o["dD"] = padded((rng.integers(-1024, 1025, (P, C)) / 256.0).astype(f32), o["ldd"])
        o["dP"] = padded((rng.integers(-1024, 1025, (G, C)) / 256.0 + 8.0).astype(f32), o["ldp"])
        arg = rng.integers(0, K, (G, C)).astype(i32)
        arg[:, 0::3], arg[:, 1::3] = 0, K - 1
        o["arg"] = np.full((G, o["lda"]), 0x7FFFFFFF, i32)
        o["arg"][:, :C], o["arg"][:, C:c4] = arg, 0
        o["Y"] = padded(nrm(P, C), o["ldy"])
        o["aff"] = block(nrm(C) * f32(0.3), np.ones(C, f32), np.zeros(C, f32), rng.uniform(0.5, 2.0, C).astype(f32))
        return o
    if kind == "multi":
        P, N, mode = d["P"], d["N"], d["mode"]
        srcs = []
        for K, ld, act in MULTI_TABLE:
            aff = None
            if act != "id":
                gamma = rng.uniform(0.5, 1.5, K) * np.where(np.arange(K) % 3 == 1, -1.0, 1.0)
                invstd = rng.uniform(0.5, 2.0, K)
                aff = block(nrm(K) * f32(0.1), (gamma * invstd).astype(f32), nrm(K), invstd.astype(f32))
            srcs.append((padded(nrm(P, K), ld), ld, K, aff, act == "relu"))
        Kt = sum(s[2] for s in srcs)
        off, c4 = 5, round4(N)
        o = dict(d, srcs=srcs, Ktot=Kt, off=off, ldw=off + Kt + 3, ldy=c4 + 4, ldg=c4 + 4, ldz=c4 + 8,
                 rpg={"rpg1": 1, "nog": 1, "one": P}[mode], stats=mode != "one")
        o["Wfull"] = np.full((N, o["ldw"]), np.nan, f32)
        o["Wfull"][:, off:off + Kt] = nrm(N, Kt) / f32(Kt ** 0.5)
        o["W"] = o["Wfull"][:, off:off + Kt]
        o["bias"] = nrm(N)
        o["gbias"] = None if mode == "nog" else padded(nrm(P // o["rpg"], N), o["ldg"])
        o["dZ"] = padded(nrm(P, N), o["ldz"])
        o["coef"] = block(nrm(N) * f32(0.5) + f32(1), nrm(N) * f32(1e-3), nrm(N) * f32(1e-3), nrm(N) * f32(0.1))
        return o
    raise KeyError(kind)


# ================================================================================================ float32 emulations

def emulate_transform(o, trans, mutant=None):
    """point_transform_kernel<trans>: T_b staged as a zero-padded [kp, kp] matrix, one fma chain per output element over the
    kp input columns in order; every quad of round4(k) columns is stored.  Returns the output buffer (SENTINEL start)."""
    B, N, k = o["B"], o["N"], o["k"]
    kp = round4(k)
    X, ldo = (o["D"], o["lddx"]) if trans else (o["X"], o["ldo"])
    sT = np.zeros((B, kp, kp), f32)
    sT[:, :k, :k] = o["T"].transpose(0, 2, 1) if trans else o["T"]
    if trans and mutant == "t_untransposed" and k % 4:
        m = np.zeros((kp, kp), bool)
        m[k & ~3:, :] = m[:, k & ~3:] = True
        m[k:, :] = m[:, k:] = False
        sT[:, m] = np.pad(o["T"], ((0, 0), (0, kp - k), (0, kp - k)))[:, m]
    x = X[:, :kp].reshape(B, N, kp)
    acc = np.zeros((B, N, kp), f32)
    for i in range(kp):
        acc = fma32(x[:, :, i:i + 1], sT[:, i:i + 1, :], acc)
    out = sentinel(B * N, ldo)
    keep = np.ones(N, bool)
    if mutant == "slab_last_row":
        keep[np.minimum(np.arange(0, N, SLAB) + SLAB, N) - 1] = False
    rows = (np.arange(B)[:, None] * N + np.nonzero(keep)[0][None, :]).reshape(-1)
    out[rows, :kp] = acc[:, keep].reshape(-1, kp)
    return out


def emulate_dt(o, mutant=None):
    """point_transform_dt_part_kernel + slab_sum_kernel: per slab, the rows dealt to 256 / blocks lanes (one lane from 256 blocks
    on), each lane one fma chain per element in row order, lanes added in lane order, slabs added in slab order starting from 0.
    Returns (dT [B, k, k] float32, workspace with its guard as float32)."""
    B, N, k = o["B"], o["N"], o["k"]
    kp = round4(k)
    _, _, _, nblk, lanes, _, _ = transform_geometry(k)
    nch = cdiv(N, SLAB)
    x = o["X"][:, :kp].reshape(B, N, kp)
    dd = o["D"][:, :kp].reshape(B, N, kp)
    ws = np.full(B * nch * k * k + 2 * MAX_K * 4, np.nan, f32)
    ws[B * nch * k * k:] = np.int32(SENTINEL).view(f32)
    part = np.zeros((B, nch, kp, kp), f32)
    for ch in range(nch):
        n0, n1 = ch * SLAB, min(ch * SLAB + SLAB, N)
        if mutant == "slab_last_row":
            n1 -= 1
        acc = np.zeros((lanes, B, kp, kp), f32)
        for t in range(cdiv(max(n1 - n0, 0), lanes)):
            for l in range(lanes):
                n = n0 + t * lanes + l
                if n < n1:
                    acc[l] = fma32(x[:, n, :, None], dd[:, n, None, :], acc[l])
        s = acc[0]
        for l in range(1, lanes):
            s = s + acc[l]
        part[:, ch] = s
    for b in range(B):                       # the stores, slab after slab (a later slab overwrites what an earlier one spilled)
        for ch in range(nch):
            base = (b * nch + ch) * k * k
            rows = kp if mutant == "dt_store_past" else k
            ws[base:base + rows * k] = part[b, ch, :rows, :k].reshape(-1)
    dT = np.zeros((B, k * k), f32)
    for ch in range(nch - 1 if mutant == "last_slab" else nch):
        dT = dT + np.stack([ws[(b * nch + ch) * k * k:(b * nch + ch + 1) * k * k] for b in range(B)])
    return dT.reshape(B, k, k), ws


def emulate_bn_max(o, mutant=None):
    """bn_max_kernel: 64 row lanes keep (max, first k) of the rows k = lane, lane + 64, ... (strict >), an idle lane (-inf, 0);
    the lanes are folded in lane order with "greater, or equal and smaller k".  Returns (out, arg) buffers (SENTINEL start)."""
    G, K, C = o["G"], o["K"], o["C"]
    c4 = round4(C)
    a = o["aff"].reshape(4, -1)
    y = o["Y"][:, :c4].reshape(G, K, c4)
    z = fma32((y - a[0]).astype(f32), a[1], a[2])
    T = cdiv(K, 64)
    zp = np.full((G, T * 64, c4), -np.inf, f32)
    zp[:, :K] = z
    zp = zp.reshape(G, T, 64, c4)
    if mutant == "last_k":
        t = T - 1 - zp[:, ::-1].argmax(1)
    else:
        t = zp.argmax(1)
    best = zp.max(1)                                                  # [G, 64, c4]
    bk = np.where(np.isneginf(best), 0, t * 64 + np.arange(64)[None, :, None])
    bv, bkk = best[:, 0], bk[:, 0]
    for l in range(1, 64):
        ov, ok = best[:, l], bk[:, l]
        if mutant == "no_smaller_k":
            take = ov > bv
        elif mutant == "idle_lane":
            take = (ov > bv) | (ok < bkk)
        else:
            take = (ov > bv) | ((ov == bv) & (ok < bkk))
        bv, bkk = np.where(take, ov, bv), np.where(take, ok, bkk)
    out, arg = sentinel(G, o["ldo"]), sentinel(G, o["ldo"]).view(i32)
    out[:G, :c4], arg[:G, :c4] = bv, bkk
    return out, arg


def _replicas(vals_by_wg, C, mutant):
    """vals_by_wg [(workgroup row, [2, C] fp64)] -> the PN2_STAT_REPLICAS x 2 x C block (replica = workgroup row % 8)."""
    red = np.zeros((STAT_REPLICAS, 2, C), f64)
    for wg, v in vals_by_wg:
        red[wg % STAT_REPLICAS] += v
    if mutant == "replica_missing":
        red[[i for i in range(STAT_REPLICAS) if red[i].any()][-1]] = 0.0
    return red.reshape(-1)


def emulate_pool_bwd(o, mutant=None):
    """pool_bwd_noact_kernel: dZp[g, c] = dOut[g ld_dout + c] (pad lanes 0), the two fp64 sums of float32 terms per workgroup
    row (four group lanes, grid rows min(cdiv(G, 4), 1024))."""
    G, K, C, ldo = o["G"], o["K"], o["C"], o["ldo"]
    c4 = round4(C)
    a = o["aff"].reshape(4, -1)
    ldg = ldo if mutant == "pitch_for_width" else o["ld_dout"]
    d = np.take(o["dOut"], np.arange(G)[:, None] * ldg + np.arange(C)[None, :], mode="clip")
    dzp = sentinel(G, ldo)
    dzp[:G, :c4] = 0.0
    dzp[:G, :C] = d
    y = o["Y"][:, :C].reshape(G, K, C)
    ys = np.take_along_axis(y, o["arg"][:, None, :C].astype(np.int64), 1)[:, 0]
    term = (d * ((ys - a[0, :C]) * a[3, :C]).astype(f32)).astype(f32)
    gy = min(cdiv(G, 4), 1024)
    wg = (np.arange(G) // 4) % gy
    vals = [(w, np.stack([d[wg == w].astype(f64).sum(0), term[wg == w].astype(f64).sum(0)])) for w in range(min(gy, 16))]
    if gy > 16:                                  # (the replica of a workgroup row is wg % 8: fold the rest in by replica)
        for r in range(STAT_REPLICAS):
            m = (wg >= 16) & (wg % STAT_REPLICAS == r)
            vals.append((r, np.stack([d[m].astype(f64).sum(0), term[m].astype(f64).sum(0)])))
    return dzp, _replicas(vals, C, mutant)


def _chain(x, w, acc):
    for i in range(x.shape[1]):
        acc = fma32(x[:, i:i + 1], w[None, :, i], acc)
    return acc


def emulate_gbias(o, cus=NOMINAL_CUS, mutant=None):
    """pn2_conv1x1_fwd (an fma chain over K, then the bias) + add_gbias_kernel (y += gbias[p / rpg] in float32; stats in fp64 of
    the stored y per workgroup row range)."""
    P, K, N, rpg = o["P"], o["K"], o["N"], o["rpg"]
    c4 = round4(N)
    y = (_chain(o["X"][:, :K], o["W"], np.zeros((P, N), f32)) + o["bias"]).astype(f32)
    p = np.arange(P)
    gi = (np.maximum(p - 1, 0) if mutant == "gbias_late" else p) // rpg
    y = (y + o["gbias"][gi, :N]).astype(f32)
    rows = row_range(cus, P, N, 16)
    keep = np.ones(P, bool)
    if mutant == "slab_last_row":
        keep[np.minimum(np.arange(0, P, rows) + rows, P) - 1] = False
        y[~keep] = (y[~keep] - o["gbias"][gi[~keep], :N]).astype(f32)
    Y = sentinel(P, o["ldy"])
    Y[:P, :c4] = 0.0
    Y[:P, :N] = y
    yd = np.where(keep[:, None], y.astype(f64), 0.0)
    vals = [(w, np.stack([yd[w * rows:(w + 1) * rows].sum(0), (yd[w * rows:(w + 1) * rows] ** 2).sum(0)])) for w in range(cdiv(P, rows))]
    return Y, _replicas(vals, N, mutant)


def emulate_colsum(o, mutant=None):
    """colsum_part_kernel + slab_sum_kernel: per slab four row lanes (r = lane, lane + 4, ...) each adding
    fma(c0, dz, fma(q1, y - mean, q0)) in row order, the lanes added ((0 + 1) + 2) + 3, the slabs in slab order from 0."""
    G, rpg, C, lds = o["G"], o["rpg"], o["C"], o["lds"]
    c4 = round4(C)
    c = o["coef"].reshape(4, c4)
    dz, y = o["dZ"][:, :c4].reshape(G, rpg, c4), o["Y"][:, :c4].reshape(G, rpg, c4)
    term = fma32(np.broadcast_to(c[0], dz.shape), dz, fma32(np.broadcast_to(c[1], y.shape), (y - c[3]).astype(f32), np.broadcast_to(c[2], y.shape)))
    nch = cdiv(rpg, SLAB)
    parts = []
    for ch in range(nch):
        r0, r1 = ch * SLAB, min(ch * SLAB + SLAB, rpg)
        if mutant == "slab_last_row":
            r1 -= 1
        lane = []
        for l in range(4):
            s = np.zeros((G, c4), f32)
            for r in range(r0 + l, r1, 4):
                s = s + term[:, r]
            lane.append(s)
        parts.append(((lane[0] + lane[1]) + lane[2]) + lane[3])
    s = np.zeros((G, c4), f32)
    for ch in range(nch - 1 if mutant == "last_slab" else nch):
        s = s + parts[ch]
    w = min(lds, c4)
    out = np.full(G * lds + 64, SENTINEL, i32).view(f32)
    o2 = out[:G * lds].reshape(G, lds)
    o2[:, :w] = s[:, :w]
    return out


def emulate_dense(o, cus=NOMINAL_CUS, mutant=None, alias=False):
    """bn_bwd_noact_dense_kernel: a workgroup's row range, four row lanes stepping four rows with (g, k) advanced incrementally."""
    G, K, C, P = o["G"], o["K"], o["C"], o["P"]
    c4 = round4(C)
    a = o["aff"].reshape(4, -1)
    rows = row_range(cus, P, C, 64)
    gg, kk = np.zeros(P, np.int64), np.zeros(P, np.int64)
    done = np.ones(P, bool)
    for p0 in range(0, P, rows):
        p1 = min(p0 + rows, P)
        if mutant == "slab_last_row":
            done[p1 - 1] = False
        for rl in range(4):
            p = p0 + rl
            g, k = p // K, p % K
            while p < p1:
                gg[p], kk[p] = g, k
                p += 4
                k += 4
                if mutant == "if_advance":
                    if k >= K:
                        k -= K
                        g += 1
                else:
                    while k >= K:
                        k -= K
                        g += 1
    gc = np.minimum(gg, G - 1)
    hit = o["arg"][gc, :c4] == kk[:, None]
    v = (o["dD"][:, :c4] + np.where(hit, o["dP"][gc, :c4], f32(0))).astype(f32)
    v[:, C:] = 0.0
    term = (v * ((o["Y"][:, :c4] - a[0]) * a[3]).astype(f32)).astype(f32)
    ldz = o["ldd"] if alias else o["ldz"]
    dZ = sentinel(P, ldz)
    if alias:
        dZ[:P] = o["dD"]
    dZ[:P][done, :c4] = v[done]
    vd, td = np.where(done[:, None], v.astype(f64), 0.0)[:, :C], np.where(done[:, None], term.astype(f64), 0.0)[:, :C]
    vals = [(w, np.stack([vd[w * rows:(w + 1) * rows].sum(0), td[w * rows:(w + 1) * rows].sum(0)])) for w in range(cdiv(P, rows))]
    return dZ, _replicas(vals, C, mutant)


def _act32(o):
    out = []
    for X, ldx, K, aff, relu in o["srcs"]:
        x = X[:, :K]
        if aff is not None:
            a = aff.reshape(4, -1)
            x = fma32((x - a[0, :K]).astype(f32), np.broadcast_to(a[1, :K], x.shape), np.broadcast_to(a[2, :K], x.shape))
            if relu:
                x = np.maximum(x, f32(0))
        out.append(x)
    return np.concatenate(out, 1)


def _dy32(o, Y):
    M, c4 = o["N"], round4(o["N"])
    c = o["coef"].reshape(4, c4)[:, :M]
    dz, y = o["dZ"][:, :M], Y[:o["P"], :M]
    return fma32(np.broadcast_to(c[0], dz.shape), dz, fma32(np.broadcast_to(c[1], y.shape), (y - c[3]).astype(f32), np.broadcast_to(c[2], y.shape)))


def emulate_multi(o, Y_in=None):
    """The three multi-source GEMMs as plain float32 chains: Y (+ stats from fp32 column sums), dW / dbias summed over the rows
    in order, dX_i chains over M.  Y_in: the Y the backward reads (default: the emulated forward)."""
    P, N = o["P"], o["N"]
    c4 = round4(N)
    A = _act32(o)
    y = (_chain(A, o["W"], np.zeros((P, N), f32)) + o["bias"]).astype(f32)
    if o["gbias"] is not None:
        y = (y + np.repeat(o["gbias"][:, :N], o["rpg"], 0)).astype(f32)
    Y = sentinel(P, o["ldy"])
    Y[:P, :c4] = 0.0
    Y[:P, :N] = y
    s = np.zeros((2, N), f32)
    for p in range(P):
        s[0] += y[p]
        s[1] = fma32(y[p], y[p], s[1])
    stats = np.zeros((STAT_REPLICAS, 2, N), f64)
    stats[0] = s
    Yb = Y if Y_in is None else Y_in
    dY = _dy32(o, Yb)
    dW = np.zeros((N, o["Ktot"]), f32)
    db = np.zeros(N, f32)
    for p in range(P):
        dW = fma32(dY[p][:, None], A[p][None, :], dW)
        db = db + dY[p]
    dX, k0 = [], 0
    for X, ldx, K, _, _ in o["srcs"]:
        buf = sentinel(P, ldx)
        buf[:P, :K] = _chain(dY, o["W"][:, k0:k0 + K].T, np.zeros((P, K), f32))
        dX.append(buf)
        k0 += K
    return Y, stats.reshape(-1), dW, db, dX


# ================================================================================================ the checks of the GPU test

def _within(got, want, bnd, what, bad):
    got = np.asarray(got, f64)
    if not np.isfinite(got).all():
        bad.append("%s: not finite" % what)
    elif not (np.abs(got - want) <= bnd).all():
        bad.append("%s: %.3g of its bound" % (what, float((np.abs(got - want) / np.maximum(bnd, 1e-300)).max())))


def _framed(buf, P, C, what, bad, zero_to=None):
    """Rows >= P and columns >= zero_to (default round4(C)) are SENTINEL, [C, zero_to) are +0.0, [0, C) are written."""
    z = round4(C) if zero_to is None else zero_to
    if not is_sentinel(buf[P:]).all():
        bad.append("%s: a row >= %d was written" % (what, P))
    if not is_sentinel(buf[:P, z:]).all():
        bad.append("%s: a column >= %d was written" % (what, z))
    if is_sentinel(buf[:P, :C]).any():
        bad.append("%s: an element was not written" % what)
    if np.ascontiguousarray(buf[:P, C:z]).view(i32).any():
        bad.append("%s: pad columns [%d, %d) are not +0.0" % (what, C, z))


def check_transform(o, out):
    bad = []
    P, k = o["B"] * o["N"], o["k"]
    ref, b = point_transform(o["X"], o["ldx"], o["T"], o["B"], o["N"], k)
    _framed(out, P, k, "out", bad)
    _within(out[:P, :k], ref, b, "out", bad)
    return bad


def check_transform_bwd(o, dX=None, dT=None, ws=None, dT2=None):
    bad = []
    B, N, k = o["B"], o["N"], o["k"]
    rdx, bdx, rdt, bdt = point_transform_bwd(o["D"], o["ldd"], o["X"], o["ldx"], o["T"], B, N, k)
    if dX is not None:
        _framed(dX, B * N, k, "dX", bad)
        _within(dX[:B * N, :k], rdx, bdx, "dX", bad)
    if dT is not None:
        _within(dT, rdt, bdt, "dT", bad)
        n = point_transform_workspace_bytes(B, N, k) // 4
        if not is_sentinel(ws[n:]).all():
            bad.append("workspace: written behind its %d bytes" % (4 * n))
        if dT2 is not None and not np.array_equal(dT.view(i32), dT2.view(i32)):
            bad.append("dT: two launches differ")
    return bad


def check_bn_max(o, out, arg=None):
    bad = []
    G, K, C = o["G"], o["K"], o["C"]
    ro, ra = bn_max(o["Y"], o["ldy"], o["aff"], G, K, C)
    assert np.array_equal(ro.astype(f32).astype(f64), ro)               # the lattice: exact in float32
    _framed(out, G, C, "out", bad)
    if not np.array_equal(out[:G, :C].view(i32), ro.astype(f32).view(i32)):
        bad.append("out: %d elements differ in bits" % int((out[:G, :C].view(i32) != ro.astype(f32).view(i32)).sum()))
    if arg is not None:
        _framed(arg.view(f32), G, C, "arg", bad)
        if not np.array_equal(arg[:G, :C], ra):
            bad.append("arg: %d elements differ" % int((arg[:G, :C] != ra).sum()))
    return bad


def check_pool_bwd(o, dzp, red):
    bad = []
    G, K, C = o["G"], o["K"], o["C"]
    d, r0, b0, r1, b1 = pool_bwd_reduce_noact(o["dOut"], o["ld_dout"], o["arg"], o["ldo"], o["Y"], o["ldy"], o["aff"], G, K, C)
    _framed(dzp, G, C, "dZp", bad)
    if not np.array_equal(dzp[:G, :C].view(i32), d.view(i32)):
        bad.append("dZp: not a copy of dOut")
    r = red_total(red, C)
    if not np.array_equal(r[0], r0):                                   # (dyadic dOut: exact in fp64 in any order)
        bad.append("red0: not exact")
    _within(r[0], r0, b0, "red0", bad)
    _within(r[1], r1, b1, "red1", bad)
    return bad


def check_gbias(o, Y, stats=None):
    bad = []
    P, K, N = o["P"], o["K"], o["N"]
    ref, b = conv1x1_fwd_gbias(o["X"], o["ldx"], o["W"], o["bias"], o["gbias"], o["ldg"], o["rpg"], P, K, N)
    _framed(Y, P, N, "Y", bad)
    _within(Y[:P, :N], ref, b, "Y", bad)
    if stats is not None:
        s, yd = red_total(stats, N), Y[:P, :N].astype(f64)
        _within(s[0], yd.sum(0), (P + 8) * U64 * np.abs(yd).sum(0), "sum y", bad)
        _within(s[1], (yd * yd).sum(0), (P + 8) * U64 * (yd * yd).sum(0), "sum y^2", bad)
    return bad


def check_colsum(o, s, s2=None):
    bad = []
    G, rpg, C, lds = o["G"], o["rpg"], o["C"], o["lds"]
    ref, b = group_colsum(o["dZ"], o["ldz"], o["Y"], o["ldy"], o["coef"], o["P"], rpg, C)
    w = min(lds, round4(C))
    body = np.ascontiguousarray(s[:G * lds].reshape(G, lds))
    if not is_sentinel(s[G * lds:]).all() or not is_sentinel(body[:, w:]).all():
        bad.append("s: written outside [G, min(lds, round4(C))]")
    if body[:, C:w].view(i32).any():
        bad.append("s: pad columns are not +0.0")
    _within(body[:, :C], ref, b, "s", bad)
    if s2 is not None and not np.array_equal(s.view(i32), s2.view(i32)):
        bad.append("s: two launches differ")
    return bad


def check_dense(o, dZ, red, alias=False):
    bad = []
    G, K, C, P = o["G"], o["K"], o["C"], o["P"]
    ref, r0, b0, r1, b1 = bn_bwd_reduce_noact_dense(o["dD"], o["ldd"], o["dP"], o["ldp"], o["arg"], o["lda"], o["Y"], o["ldy"], o["aff"], G, K, C)
    assert np.array_equal(ref.astype(f32).astype(f64), ref)             # dyadic operands: the addition is exact
    c4 = round4(C)
    if alias:                                                           # (dZ lives in dDense's buffer: its NaN tail stays)
        if not is_sentinel(dZ[P:]).all() or not np.isnan(dZ[:P, c4:]).all():
            bad.append("dZ: written outside [P, round4(C)]")
        if np.ascontiguousarray(dZ[:P, C:c4]).view(i32).any():
            bad.append("dZ: pad columns are not +0.0")
    else:
        _framed(dZ, P, C, "dZ", bad)
    if not np.array_equal(np.ascontiguousarray(dZ[:P, :C]).view(i32), ref.astype(f32).view(i32)):
        bad.append("dZ: %d elements differ in bits" % int((np.ascontiguousarray(dZ[:P, :C]).view(i32) != ref.astype(f32).view(i32)).sum()))
    r = red_total(red, C)
    if not np.array_equal(r[0], r0):
        bad.append("red0: not exact")
    _within(r[1], r1, b1, "red1", bad)
    return bad


def check_multi(o, Y, stats, dW, db, dX):
    """dW: the [N + 2, ldw] frame whose [:N, off : off + Ktot] window is accumulated from zero; the rest stays zero."""
    bad = []
    P, N, Kt, off = o["P"], o["N"], o["Ktot"], o["off"]
    ref, b = conv1x1_fwd_multi(o["srcs"], o["W"], o["bias"], o["gbias"], o["ldg"], o["rpg"], P, N)
    _framed(Y, P, N, "Y", bad)
    _within(Y[:P, :N], ref, b, "Y", bad)
    if stats is not None:
        s, yd = red_total(stats, N), Y[:P, :N].astype(f64)
        _within(s[0], yd.sum(0), bound(P, np.abs(yd).sum(0)), "sum y", bad)
        _within(s[1], (yd * yd).sum(0), bound(P, (yd * yd).sum(0), 1), "sum y^2", bad)
    if bad:
        return bad                                                       # (the backward reads this Y)
    rW, bW, rb, bb = conv1x1_wgrad_multi(o["dZ"], o["ldz"], Y, o["ldy"], o["coef"], o["srcs"], P, N)
    _within(dW[:N, off:off + Kt], rW, bW, "dW", bad)
    frame = dW.copy()
    frame[:N, off:off + Kt] = 0.0
    if frame.view(i32).any():
        bad.append("dW: written outside its window")
    _within(db, rb, bb, "dbias", bad)
    for i, ((r, bd), buf, src) in enumerate(zip(conv1x1_dgrad_multi(o["dZ"], o["ldz"], Y, o["ldy"], o["coef"], o["W"], [s[2] for s in o["srcs"]], P, N), dX, o["srcs"])):
        K = src[2]
        _framed(buf, P, K, "dX[%d]" % i, bad, zero_to=K)
        _within(buf[:P, :K], r, bd, "dX[%d]" % i, bad)
    return bad
