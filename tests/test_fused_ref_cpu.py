"""tests/fused_ref.py checked without a GPU: (a) a float32 RESTATEMENT of what the two kernels compute -- padded tiles, zero
padded weights, bias, ReLU, the three pooling forms -- stays inside the running a-priori bound against the fp64 statement
for every case of the GPU files (pn2_group_conv_fwd at 6 slabs instead of 8 C and more), evaluated twice: the dot products
by CPU torch, and by a sequential-order float32 accumulation in numpy (one rounding per product and per addition); (b) six
mistakes a kernel of this kind can make, put into the restatement (never into a kernel), each break the tolerance of
tests/test_group_conv_gpu.py / tests/test_fused_eval_gpu.py that its case uses, while the clean restatement keeps it.

The tolerance functions are the ones the GPU files call (fused_ref.group_conv_errors / group_conv_ok, eval_errors /
eval_ok), so what is shown here is shown for the assertions that run on the device.

The tiles of the restatement start as NaN, like memory nobody has written: with zero padded weights a FINITE value in a pad
column between two layers is harmless (0 * finite), what breaks a result is a pad column that is never written, and that
is how the mutation "a nonzero pad column" is stated.

Measured here (CPU torch / sequential numpy): worst |err| / bound 0.27 / 0.27 over the pn2_fused_eval cases (the narrow
g16_k3_13; 2e-5 on 520 -> 256 -> 128 -> 13), 0.49 / 0.47 over the pn2_group_conv_fwd shapes.  The mutations leave the bound
by: a dropped k column 3.6 (520 wide last layer), 4.1 (the deep wide chain) .. 1.9e6; centre after the multiply 3.0 .. 20
(pn2_fused_eval, KITTI scale), 3e3 (pn2_group_conv_fwd); the wrong 16 rows 3.6e3 .. 2.9e6; a missing ReLU 2e4 .. 1.6e5; a
stale slab 5e6 with 576 elements of X differing; an unwritten pad column: NaN.  The file takes 3 s.
"""
import numpy as np
import pytest
import torch

import fused_ref as R

DEV = torch.device("cpu")
F32 = np.float32


# ------------------------------------------------------------------------------------------------ the restatement

def _mm(a, W, mode):
    """a [P, K] @ W [N, K]^T in float32: CPU torch, or sequentially over k in numpy."""
    if mode == "torch":
        return a @ W.t()
    an, Wn = a.numpy().astype(F32), W.numpy().astype(F32)
    acc = np.zeros((an.shape[0], Wn.shape[0]), F32)
    for k in range(an.shape[1]):
        acc = acc + an[:, k:k + 1] * Wn[None, :, k]
    assert acc.dtype == F32
    return torch.from_numpy(acc)


def _nan_tile(P, cols):
    return torch.full((P, cols), R.SENTINEL, dtype=torch.int32).view(torch.float32)


def _raw_and_centre(geo, xyz_first):
    """Un-centred grouped rows [P, 3 + D] and, in the same columns, the centre of every row (zero in the feature columns)."""
    B, N, S, K, D = geo["B"], geo["N"], geo["S"], geo["K"], geo["D"]
    rows = (geo["idx"] + torch.arange(B).view(B, 1, 1) * N).reshape(-1)
    xo, fo = (0, 3) if xyz_first else (D, 0)
    raw, cen = torch.zeros(B * S * K, 3 + D), torch.zeros(B * S * K, 3 + D)
    raw[:, xo:xo + 3] = geo["xyz"].reshape(B * N, 3)[rows]
    cen[:, xo:xo + 3] = geo["new_xyz"].reshape(B * S, 1, 3).expand(B * S, K, 3).reshape(-1, 3)
    if D:
        raw[:, fo:fo + D] = geo["points"].reshape(B * N, D)[rows]
    return raw, cen


def restate_eval(st, mode, mutate=None):
    """pn2_fused_eval on the operands of a fused_ref.eval_case in float32, as csrc/eval.hip lays it out: rows padded to
    round8(K) columns, weights read up to round8(K) of their storage, hidden tiles written as relu(acc + b) with zero pad
    columns, the last layer pooled (max of the accumulators, then + b, then relu) or stored."""
    layers, pool, K0, P = st["layers"], st["pool"], st["K0"], st["P"]
    a = _nan_tile(P, R.round8(K0))
    a[:, :K0], a[:, K0:] = st["X"][:, :K0], 0.0
    for l, (W, b, store, ldw) in enumerate(layers):
        N, K = W.shape
        K8 = R.round8(K)
        Wp = store[:, :K8].clone()                                  # (the zero pad of the storage is part of what is read)
        last = l == len(layers) - 1
        if mutate == "drop_k" and last:
            Wp[:, K // 2] = 0.0
        if mutate == "late_centre" and l == 0:
            raw, cen = _raw_and_centre(st["geo"], st["xyz_first"])
            acc = _mm(torch.cat([raw, a[:, K0:]], 1), Wp, mode) - _mm(torch.cat([cen, a[:, K0:]], 1), Wp, mode)
        else:
            acc = _mm(a, Wp, mode)
        if not last:
            z = acc + b
            a = _nan_tile(P, R.round8(N))
            a[:, :N] = z if (mutate == "no_relu" and l == 0) else torch.relu(z)
            if not (mutate == "pad_unwritten" and N % 8):
                a[:, N:] = 0.0
            continue
        if pool == 0:
            return torch.relu(acc + b)
        if mutate == "wrong_half":
            assert pool == 16
            whole = P // 32 * 32                                    # tiles that hold two groups: each takes the other's rows
            acc = torch.cat([acc[:whole].view(-1, 2, 16, N).flip(1).reshape(whole, N), acc[whole:]])
        return torch.relu(acc.view(-1, pool, N).amax(1) + b)


def restate_group_conv(case, st, xyz_first, ldx, mode, mutate=None, stride=2):
    """pn2_group_conv_fwd in float32: X as the kernel puts it together (gather, one subtraction, copies, zero pads), Y = X W^T
    + b, the sums from the float32 Y.  stale_slab: the rows of the last slab are the gather of the slab `stride` earlier."""
    geo, W, b = case["geo"], case["W"], case["bias"]
    ci = W.shape[1]
    raw, cen = _raw_and_centre(geo, xyz_first)
    X = torch.zeros(raw.shape[0], ldx)
    X[:, :ci] = raw - cen
    if mutate == "stale_slab":
        s = X.shape[0] // 64 - 1
        X[64 * s:64 * s + 64] = X[64 * (s - stride):64 * (s - stride) + 64].clone()
    if mutate == "late_centre":
        Y = _mm(raw, W, mode) - _mm(cen, W, mode) + b
    else:
        Y = _mm(X[:, :ci], W, mode) + b
    Yd = Y.double()
    return X, Y, torch.stack([Yd.sum(0), (Yd * Yd).sum(0)])


# ------------------------------------------------------------------------------------------------ (a) clean restatement

ALL_EVAL = dict(R.EVAL_CASES, lds_limit_636=dict(rows=33, K0=636, ldx=636, widths=[13], pool=0))


@pytest.mark.parametrize("name", list(ALL_EVAL))
def test_eval_restatement_stays_inside_the_bound(name):
    st = R.eval_case(DEV, name, ALL_EVAL[name])
    for mode in ("torch", "seq"):
        e = R.eval_errors(st, restate_eval(st, mode)).tolist()
        print("%-24s %-5s err %.3e  e32 %.3e  err/bound %.4f" % (name, mode, e[2], st["e32"], e[1]))
        assert e[0] == 0, (name, mode, "outside the running bound", e)
        if mode == "torch":
            assert R.eval_ok(st, e), (name, e)
    if st.get("dead") is not None:
        assert bool((st["ref"][:, st["dead"]] == 0).all()) and bool((restate_eval(st, "torch")[:, st["dead"]] == 0).all())


def test_statement_of_the_grouped_rows():
    """One rounding per centred element, features copied, pads zero, index with 0, N - 1 and duplicates in every cloud."""
    geo = R.draw_geometry(DEV, 3, 50, 4, 16, 6, 3, kitti=True)
    for b in range(3):
        flat = geo["idx"][b].reshape(-1)
        assert int(flat.min()) == 0 and int(flat.max()) == 49 and int(flat[1]) == int(flat[2]) == int(flat[32])
    for xyz_first in (0, 1):
        X, x64, E0 = R.grouped_rows(geo, xyz_first, 12)
        raw, cen = _raw_and_centre(geo, xyz_first)
        assert torch.equal(X[:, :9], raw - cen) and bool((X[:, 9:] == 0).all())
        assert torch.equal(x64, raw.double() - cen.double())
        xo = 0 if xyz_first else 6
        assert bool((E0[:, xo:xo + 3] == R.U32 * x64[:, xo:xo + 3].abs()).all()) and float(E0.sum()) == float(E0[:, xo:xo + 3].sum())
        assert float(x64[:, xo:xo + 3].abs().max()) < 3e-3 and float(raw.abs().max()) > 60      # KITTI scale, centred magnitudes


@pytest.mark.parametrize("K", R.GROUP_CONV_K)
@pytest.mark.parametrize("co,D", R.GROUP_CONV_CD)
def test_group_conv_restatement_keeps_the_tolerance(co, D, K):
    slabs, worst = 6, {"torch": 0.0, "seq": 0.0}
    B, S = 2, 64 * slabs // K // 2
    for kitti in (False, True):
        case = R.group_conv_case(DEV, B, S, K, D, co, 10 * K + D, kitti=kitti, ldw_extra=5)
        for xyz_first, ldx in ((0, R.round4(3 + D)), (1, 12)):
            st = R.group_conv_statement(case, xyz_first, ldx)
            for mode in ("torch", "seq"):
                X, Y, sums = restate_group_conv(case, st, xyz_first, ldx, mode)
                e = R.group_conv_errors(st, X, Y, sums).tolist()
                assert R.group_conv_ok(e), (kitti, xyz_first, ldx, mode, e)
                worst[mode] = max(worst[mode], e[2])
    print("C_out %d D %d K %d: err/bound %.3f (torch) %.3f (sequential)" % (co, D, K, worst["torch"], worst["seq"]))


# ------------------------------------------------------------------------------------------------ (b) mutations

EVAL_MUTATIONS = [("drop_k", "g32_k4_33_33"), ("drop_k", "g16_k3_13"), ("drop_k", "rows33_deep_wide"), ("drop_k", "g96_k12_8_13_33_520"),
                  ("late_centre", "g32_kitti_32_33"), ("late_centre", "g128_k16_kitti_40_13"),
                  ("wrong_half", "g16_k3_13"), ("wrong_half", "g16_kitti_40_520"),
                  ("no_relu", "g64_k9_32_40_160"), ("no_relu", "rows33_12_40_13"),
                  ("pad_unwritten", "g96_k12_8_13_33_520"), ("pad_unwritten", "g32_k4_33_33")]


@pytest.mark.parametrize("mutate,name", EVAL_MUTATIONS)
def test_eval_mutation_breaks_the_tolerance(mutate, name):
    st = R.eval_case(DEV, name)
    clean = R.eval_errors(st, restate_eval(st, "torch")).tolist()
    broken = R.eval_errors(st, restate_eval(st, "torch", mutate)).tolist()
    print("%-14s %-24s clean err/bound %.3f  mutated: %d elements outside, err/bound %.3g, err %.3g against 4 e32 = %.3g" %
          (mutate, name, clean[1], broken[0], broken[1], broken[2], 4 * st["e32"]))
    assert R.eval_ok(st, clean)
    assert not R.eval_ok(st, broken)
    assert broken[0] > 0                                           # (the running bound alone sees it; on 520 -> 256 -> 128 -> 13 by 4x only)


@pytest.mark.parametrize("mutate,kitti,K", [("stale_slab", False, 16), ("stale_slab", False, 96), ("late_centre", True, 32), ("late_centre", True, 3)])
def test_group_conv_mutation_breaks_the_tolerance(mutate, kitti, K):
    B, S = 2, 64 * 6 // K // 2
    case = R.group_conv_case(DEV, B, S, K, 6, 64, 77, kitti=kitti)
    st = R.group_conv_statement(case, 0, 12)
    clean = R.group_conv_errors(st, *restate_group_conv(case, st, 0, 12, "torch")).tolist()
    broken = R.group_conv_errors(st, *restate_group_conv(case, st, 0, 12, "torch", mutate)).tolist()
    print("%-12s K %d: clean %s  mutated: X elements %d, Y outside %d, err/bound %.3g" % (mutate, K, clean[:3], broken[0], broken[1], broken[2]))
    assert R.group_conv_ok(clean) and not R.group_conv_ok(broken)
    assert broken[1] > 0 and (mutate != "stale_slab" or broken[0] > 0)
