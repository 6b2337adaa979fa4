"""GPU: pn2_fused_eval (csrc/eval.hip: gather -> up to four MFMA layers in LDS -> max) called through the C ABI and held to
the fp64 statement of tests/fused_ref.py.  The folded W', b' are drawn as float32: no BatchNorm fold, no ball query and no
FPS is in the path.

Tolerance of every run (fused_ref.eval_ok): EVERY element within the derived running bound E_L, and max |err| <=
max(4 e32, 4 u max|ref|) with e32 = max |plain torch float32 chain on the same operands - fp64| (measured against torch,
never against the kernel).  The output sits in a sentinel-filled buffer of pitch ldo = round4(N_L) + 8: rows behind P
(pool == 0) or P / pool keep the sentinel; the columns [N_L, ldo) keep it for pool == 0, 16 and 32 and are ZERO for pool >
32 (the launcher clears whole rows of pitch ldo for the integer atomicMax; include/pn2.h says so).

Coverage by construction (fused_ref.EVAL_CASES; every grouped case runs with xyz_first both ways):

    case                    K_0  k loops (8-wide steps per layer)          last N: blocks / waves   pooling form
    g16_k3_13                 3  1 (remainder only)                        13: one block            16, 9 groups: last tile holds one
    g16_kitti_40_520         12  2 | 5 = 4 + 1                             520: 17 blocks           16, 15 groups, KITTI scale
    g32_k4_33_33              4  1 | 5 (hidden 33 -> round8 40)            33: one live column      32: plain store; dead channel
    g32_kitti_32_33           3  1 | 4 = exactly one group of four         33                       32, KITTI scale
    g64_k9_32_40_160          9  2 | 4 | 5 (hidden 32, 40), ldw + 8        160: 5 blocks / 4 waves  64: zero fill + atomicMax; dead channel
    g96_k12_8_13_33_520      12  2 | 1 (hidden 8) | 2 (hidden 13) | 5      520                      96 = 3 tiles per group, L = 4
    g128_k16_kitti_40_13     16  2 | 5, ldw + 4                            13                       128, KITTI scale
    group_all_33_160          9  2 | 5                                     160                      idx, new_xyz NULL, S = 1, Knb = N = 64
    rows{1,31,32,33}_12_40_13 12 2 | 5                                     13                       pool 0, ragged last tile
    rows95_16_33_160         16  2 | 5, ldw + 8, ldx 20                    160                      pool 0
    rows33_deep_wide        520  65 | 32 | 16  (520 -> 256 -> 128 -> 13)   13                       pool 0; the case the 4x rule is for
    rows96_pool32_32_8_33    32  4 | 1                                     33                       plain rows, pool 32
    test_lds_limit          633 / 636 / 637 / 640, single layer -> 13      13                       pool 0

A layer whose K is 1 .. 4 mod 8 ends in a step of four columns (the upper half-wave multiplies by zero without reading), and
a tile row then holds round4(K) columns and no more.  K_0 = 3, 4, 9, 12 and the hidden widths 33 reach that step; in
g16_k3_13 (pitch 4), g32_k4_33_33 and g96_k12_8_13_33_520 (pitch 36: the hidden 33 fills its row to the last column, and
row 31 of the second tile ends where the LDS ends) and the single-layer NaN case (pitch 12) the pitch is exactly that
width, so a quad read or a pad column written one step too far lands in the next row and leaves the bound.

NaN (test_nan_*): a NaN in one feature of one input row.  Pooled outputs are finite (the documented deviation: fmaxf and
the integer atomicMax drop it); with pool == 0 the row comes out as NaN in every column, as torch.relu has it, through a
hidden layer too, and every other row stays inside the tolerance.

THE LDS LIMIT.  The kernel keeps two [32][LP] float tiles in at most 160 KiB, LP the least pitch = 4 mod 8 that holds
round4(widest layer input) columns, so LP <= 640: K_0 = 636 (LP 636, 162 816 bytes) runs and is correct, 637 (LP 644,
164 864 > 163 840) is refused with nothing written, and pointnet_util._fused_eval_ok answers the same (test_lds_limit).
When this file was first written the tiles held round8(K) + 4 columns and 636 was refused like 637; the rows were narrowed
to round4(K) for this test, the results of every other case unchanged bit for bit (the same MFMA sequence on the same
operands: the quad that is no longer read was all zero padding).

MEASURED on an MI355X (max |err|, e32 of plain torch, worst |err| / running bound; both layouts, the larger figure):
    g16_k3_13 2.7e-7 2.7e-7 0.28 | g16_kitti_40_520 5.7e-8 5.7e-8 0.043 | g32_k4_33_33 1.2e-6 1.2e-6 0.041
    g32_kitti_32_33 2.7e-8 2.7e-8 0.033 | g64_k9_32_40_160 1.7e-6 1.8e-6 0.006 | g96_k12_8_13_33_520 2.7e-6 2.7e-6 0.006
    g128_k16_kitti_40_13 3.0e-8 2.5e-8 0.017 | group_all_33_160 1.7e-6 1.4e-6 0.042 | rows1 7.0e-8 2.3e-7 0.002
    rows31 4.6e-7 5.1e-7 0.013 | rows32 4.7e-7 5.8e-7 0.016 | rows33 7.8e-7 5.4e-7 0.021 | rows95_16_33_160 1.3e-6 1.1e-6 0.031
    rows33_deep_wide 1.7e-6 1.6e-6 0.00002 | rows96_pool32 6.6e-7 7.1e-7 0.016
    K_0 = 636 3.1e-6 1.2e-6 0.003 | K_0 = 633 3.7e-6 9.4e-7 0.004
i.e. the kernel's error is 0.3 .. 1.7 x that of torch's own float32 chain on the cases of the table (the rule allows 4 x).
The two single layers at the LDS limit come to 2.7 x and 3.9 x: there one MFMA chain adds ~636 products in sequence, where
torch's GEMM splits the sum, so the kernel's error grows like the sequential sqrt(K) u and torch's does not.  The running
bound, sharp on the short narrow chains (0.28), is four orders loose on 520 -> 256 -> 128 -> 13, which is why both are held.
The fp64 statements are formed on the GPU, one synchronisation per case: the file takes 2.5 s (23 tests).
"""
import ctypes

import pytest
import torch

import fused_ref as R
from pointnet12_amd import _lib
from pointnet12_amd import pointnet_util as U

pytestmark = pytest.mark.gpu

I32 = torch.int32


def _p(t):
    return None if t is None else t.data_ptr()


def _layer_array(layers):
    arr = (_lib.EvalLayer * len(layers))()
    for l, (W, b, store, ldw) in enumerate(layers):
        arr[l].W, arr[l].bias, arr[l].K, arr[l].N, arr[l].ldw = store.data_ptr(), b.data_ptr(), W.shape[1], W.shape[0], ldw
    return arr


def _launch(st, check=True):
    """One pn2_fused_eval call on the operands of a fused_ref.eval_case, into a sentinel-filled [rows + guard, ldo]."""
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    arr, pool, P = _layer_array(st["layers"]), st["pool"], st["P"]
    n_out = st["layers"][-1][0].shape[0]
    rows_out, ldo = (P // pool if pool else P), R.round4(n_out) + 8
    out = R.guarded(rows_out, ldo, st["X"].device)
    layers = ctypes.cast(arr, ctypes.c_void_p)
    if st["geo"] is None:
        rc = lib.pn2_fused_eval(_p(st["X"]), st["X"].shape[1], None, None, None, None, P, 0, 0, pool or 1, 0, 1, layers,
                                len(st["layers"]), pool, _p(out), ldo, stream)
    else:
        g = st["geo"]
        rc = lib.pn2_fused_eval(None, 0, _p(g["xyz"]), _p(g["points"]), _p(g["new_xyz"]), _p(g["idx"]), g["B"], g["N"], g["S"], g["K"],
                                g["D"], int(st["xyz_first"]), layers, len(st["layers"]), pool, _p(out), ldo, stream)
    assert rc == 0 or not check, rc
    return out, rows_out, n_out, rc


def _guard_misses(out, rows, n, pool):
    """Device scalar: what is wrong around the result (module docstring): rows behind `rows`, the columns [n, ldo), and
    elements inside that were never written."""
    bits = out.view(I32)
    behind = bits[:rows, n:]
    cols = (behind != 0).sum() if pool > 32 else (behind != R.SENTINEL).sum()
    return ((bits[rows:] != R.SENTINEL).sum() + cols + (bits[:rows, :n] == R.SENTINEL).sum()).double()


def _run_and_measure(st):
    out, rows, n, _ = _launch(st)
    e = torch.cat([R.eval_errors(st, out[:rows, :n]), _guard_misses(out, rows, n, st["pool"]).view(1)])
    if st.get("dead") is not None:
        e = torch.cat([e, (out[:rows, st["dead"]].contiguous().view(I32) != 0).sum().double().view(1)])
    return e


def _assert_case(st, e, tag):
    print("%-24s %-12s err %.3e  e32 %.3e  max|ref| %.3e  err/bound %.4f" % (st["name"], tag, e[2], st["e32"], st["refmax"], e[1]))
    assert e[3] == 0, (st["name"], tag, "guard elements wrong", e[3])
    assert e[0] == 0, (st["name"], tag, "elements outside the running bound", e[0], "worst err / bound", e[1])
    assert R.eval_ok(st, e), (st["name"], tag, "max err", e[2], "allowed", max(4 * st["e32"], 4 * R.U32 * st["refmax"]))
    if st.get("dead") is not None:
        assert e[4] == 0, (st["name"], tag, "pooled outputs of the dead channel that are not exactly +0", e[4])


@pytest.mark.parametrize("name", list(R.EVAL_CASES))
def test_cases(dev, name):
    """Every case of fused_ref.EVAL_CASES (module docstring), the grouped ones with xyz_first both ways."""
    sts = [R.eval_case(dev, name)]
    if sts[0]["geo"] is not None:
        sts.append(R.eval_case(dev, name, dict(R.EVAL_CASES[name], xyz_first=1 - R.EVAL_CASES[name]["xyz_first"])))
    es = torch.stack([_run_and_measure(st) for st in sts]).cpu().tolist()      # one synchronisation
    for st, e in zip(sts, es):
        _assert_case(st, e, "xyz_first %d" % st["xyz_first"] if st["geo"] is not None else "rows")


def _single_layer(K0):
    return dict(rows=33, K0=K0, ldx=R.round4(K0), widths=[13], pool=0)


def _module_says_ok(K0):
    convs = [torch.nn.Conv2d(K0, 13, 1)]
    with torch.no_grad():
        return U._fused_eval_ok(K0, convs, 0)


def _assert_refused(dev, K0):
    st = R.eval_case(dev, "lds%d" % K0, _single_layer(K0))
    out, _, _, rc = _launch(st, check=False)
    assert rc < 0
    assert int((out.view(I32) != R.SENTINEL).sum()) == 0, (K0, "a refused call wrote something")
    assert not _module_says_ok(K0)


def _assert_runs(dev, K0):
    st = R.eval_case(dev, "lds%d" % K0, _single_layer(K0))
    out, rows, n, rc = _launch(st, check=False)
    assert rc == 0, (K0, "refused", rc)
    e = torch.cat([R.eval_errors(st, out[:rows, :n]), _guard_misses(out, rows, n, 0).view(1)]).cpu().tolist()
    _assert_case(st, e, "K0 %d" % K0)
    assert _module_says_ok(K0)


def test_lds_limit(dev):
    """Two [32][LP] tiles in 160 KiB, LP the least pitch = 4 mod 8 that holds round4(K_0) columns: a single layer with K_0 =
    636 (LP 636) runs and is correct, K_0 = 637 (LP 644) is refused with nothing written, and pointnet_util._fused_eval_ok
    answers the same on both sides of the limit."""
    _assert_refused(dev, 637)
    _assert_runs(dev, 636)


def test_lds_limit_inside_the_last_pitch(dev):
    """The other ends of the two pitches around the limit: K_0 = 633 (the first width of LP 636: 79 full steps and a step of
    four columns of which one is live) runs and is correct, K_0 = 640 (the last of LP 644) is refused."""
    _assert_refused(dev, 640)
    _assert_runs(dev, 633)


@pytest.mark.parametrize("name", ["g32_k4_33_33", "g64_k9_32_40_160", "g16_kitti_40_520"])
def test_nan_is_dropped_by_the_pooling(dev, name):
    """A NaN feature of one source point (every grouped row that gathers it carries it, through the hidden layers): the pooled
    outputs are finite everywhere -- the deviation include/pn2.h documents -- and the groups that do not contain the point
    stay inside the tolerance."""
    st = R.eval_case(dev, name)
    g = st["geo"]
    j = int(g["idx"][0, 0, 3])
    g["points"][0, j, 0] = float("nan")
    hit = (g["idx"][0] == j).any(-1)                                # groups of cloud 0 that gather the point
    clean = torch.ones(g["B"] * g["S"], dtype=torch.bool, device=dev)
    clean[:g["S"]] = ~hit
    out, rows, n, _ = _launch(st)
    assert bool(torch.isfinite(out[:rows, :n]).all())
    sub = dict(st, ref=st["ref"][clean], bound=st["bound"][clean])
    e = R.eval_errors(sub, out[:rows, :n][clean]).cpu().tolist()
    assert bool(hit.any()) and R.eval_ok(sub, e), e


@pytest.mark.parametrize("name", ["rows33_12_40_13", "rows95_16_33_160", "single"])
def test_nan_shows_in_unpooled_rows(dev, name):
    """pool == 0: a NaN in one feature of one input row makes that output row NaN in every column (relu as torch.relu: x < 0 ?
    0 : x, in the hidden layers and in the store), and no other row moves."""
    st = R.eval_case(dev, "nan_single", dict(rows=33, K0=9, ldx=12, widths=[40], pool=0)) if name == "single" else R.eval_case(dev, name)
    r = st["P"] - 2
    st["X"][r, 1] = float("nan")
    out, rows, n, _ = _launch(st)
    assert bool(torch.isnan(out[r, :n]).all()), "the NaN row came out finite"
    keep = torch.arange(rows, device=dev) != r
    sub = dict(st, ref=st["ref"][keep], bound=st["bound"][keep])
    e = R.eval_errors(sub, out[:rows, :n][keep]).cpu().tolist()
    assert R.eval_ok(sub, e), e
