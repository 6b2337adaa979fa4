"""GPU: the loss tail (csrc/loss.hip) -- pn2_log_softmax_fwd / _bwd and pn2_nll_loss_fwd / _bwd -- called through the C ABI
with row pitches the Python wrappers never pass, against fp64 references of the same float32 inputs.

TOLERANCE of the two log-softmax kernels (the rule, not a measured figure): per case
    max(4 x the error of ATen's float32 kernel on the same device against the same fp64 answer,  8 * 2^-24 * max(1, max|x|)).
4 x is the margin this project gives a correct float32 evaluation elsewhere (tests/test_mlp_gpu.py, _check_shared_mlp); the
floor covers the cases in which ATen happens to be exact: a float32 result near max|x| cannot be closer to the fp64 one
than half an ulp, 2^-24 max|x|, and a handful of roundings (max, exp, sum, log, the subtraction) stack up to a few of those.
For the backward max|x| is the largest incoming gradient (or outgoing, if larger).

Every output buffer is pre-filled with a NaN pattern no kernel produces and has one spare row: what a kernel promises to
write must be written, what it does not own must still hold the pattern.
"""
import pytest
import torch
import torch.nn.functional as F

from pointnet12_amd import _lib
from pointnet12_amd import pointnet_util as U
from pointnet12_amd.loss import nll_loss

pytestmark = pytest.mark.gpu

SENT = 0x7FC0DEAD                        # a quiet-NaN bit pattern no kernel produces
I32 = torch.int32
U32 = 2.0 ** -24
CS = (1, 2, 3, 4, 5, 13, 16, 50, 63, 64)
RS = (1, 255, 256, 257, 70001)
KINDS = ("randn", "shift_up", "shift_down", "one_neg_inf", "all_equal")


def r4(c):
    return (c + 3) & ~3


def lib_st():
    return _lib.load(), torch.cuda.current_stream().cuda_stream


def sentinel(shape, dev):
    return torch.full(shape, SENT, dtype=I32, device=dev).view(torch.float32)


def is_sent(t):
    return t.contiguous().view(I32) == SENT


def _gen(seed, dev):
    return torch.Generator(device=dev).manual_seed(seed)


def _logits(kind, R, C, dev):
    g = _gen(1000 * C + R % 997, dev)
    x = torch.randn(R, C, device=dev, generator=g) * 3
    if kind == "shift_up":
        x = x + 1e4
    elif kind == "shift_down":
        x = x - 1e4
    elif kind == "one_neg_inf":
        col = torch.randint(0, C, (R,), device=dev, generator=g)
        x[torch.arange(R, device=dev), col] = float("-inf")
    elif kind == "all_equal":
        x[0] = 2.5                       # one all-equal row among ordinary ones
        x[R // 2] = -7.0
    return x


def _err(a, ref):
    """max |a - ref| over the finite entries of ref; where ref is infinite a must be the same infinity."""
    fin = torch.isfinite(ref)
    assert torch.equal(a[~fin].double(), ref[~fin])
    return float((a.double() - ref)[fin].abs().max()) if bool(fin.any()) else 0.0


def _run_fwd(x, C, ldx, ldo):
    """pn2_log_softmax_fwd on x [R, C] laid out at pitch ldx with +1e30 in the pad columns -> out [R, C] (pitch ldo checked)."""
    lib, st = lib_st()
    R = x.shape[0]
    xp = torch.full((R, ldx), 1e30, device=x.device)
    xp[:, :C] = x
    out = sentinel((R + 1, ldo), x.device)
    assert lib.pn2_log_softmax_fwd(xp.data_ptr(), ldx, R, C, out.data_ptr(), ldo, st) == 0
    assert bool(is_sent(out[R]).all()) and bool(is_sent(out[:R, C:]).all()), "wrote outside its C columns"
    assert not bool(is_sent(out[:R, :C]).any())
    return out[:R, :C]


@pytest.mark.parametrize("C", CS)
def test_log_softmax_fwd_pitches_and_edge_rows(dev, C):
    """Measured on an MI355X, worst (our error) / (ATen's float32 error) per C over the cases in which ATen is not exact:
        C                      2     3     4     5     13    16    50    63    64      (C = 1: both exact)
        unshifted rows         1.16  1.04  1.82  1.45  1.86  1.54  1.00  1.00  1.02
        rows shifted by 1e4    1135  4734  3198  3666  3058  793   2091  469   903
    On unshifted rows (randn * 3, one -inf, all equal) both err by 0.7 .. 2e-6.  On rows shifted by +-1e4 the kernel errs by
    4.9e-4 = half an ulp of 1e4 -- it forms lse = max + log(sum) and rounds it at the magnitude of the logits, where ATen forms
    (x - max) - log(sum) and stays at 1e-6.  The floor of the rule, 8 * 2^-24 * max|x| = 4.8e-3 there, admits that."""
    worst = {False: 0.0, True: 0.0}                          # unshifted / shifted rows
    for R in RS:
        for kind in KINDS:
            if kind == "one_neg_inf" and C == 1:
                continue                                     # (the whole row then: test_log_softmax_all_neg_inf_row_is_nan)
            x = _logits(kind, R, C, dev)
            ref = torch.log_softmax(x.double(), -1)
            aten = _err(torch.log_softmax(x, -1), ref)
            tol = max(4 * aten, 8 * U32 * max(1.0, float(x[torch.isfinite(x)].abs().max())))
            for ldx in (r4(C), r4(C) + 4):
                for ldo in (C, C + 3):
                    mine = _err(_run_fwd(x, C, ldx, ldo), ref)
                    print("fwd C=%d R=%d %s ldx=%d ldo=%d: ours %.3g aten %.3g tol %.3g" % (C, R, kind, ldx, ldo, mine, aten, tol))
                    assert mine <= tol, (R, kind, ldx, ldo, mine, aten, tol)
                    if aten > 0:
                        worst[kind.startswith("shift")] = max(worst[kind.startswith("shift")], mine / aten)
    print("fwd C=%d ratio unshifted %.2f shifted %.0f" % (C, worst[False], worst[True]))


def test_log_softmax_all_neg_inf_row_is_nan(dev):
    for C in (1, 5, 64):
        x = _logits("randn", 9, C, dev)
        x[4] = float("-inf")
        out = _run_fwd(x, C, r4(C), C)
        ref = torch.log_softmax(x, -1)
        assert bool(torch.isnan(ref[4]).all()) and bool(torch.isnan(out[4]).all())
        keep = torch.arange(9, device=dev) != 4
        assert _err(out[keep], torch.log_softmax(x[keep].double(), -1)) <= 8 * U32 * float(x[keep].abs().max())


def _run_bwd(g, out, C, ldg, ldo, ldgx):
    lib, st = lib_st()
    R = g.shape[0]
    gp = torch.full((R, ldg), 1e30, device=g.device)
    gp[:, :C] = g
    op = torch.full((R, ldo), 1e30, device=g.device)
    op[:, :C] = out
    gx = sentinel((R + 1, ldgx), g.device)
    assert lib.pn2_log_softmax_bwd(gp.data_ptr(), ldg, op.data_ptr(), ldo, R, C, gx.data_ptr(), ldgx, st) == 0
    assert bool(is_sent(gx[R]).all()), "wrote past its R rows"
    assert bool((gx[:R, C:].contiguous().view(I32) == 0).all()), "pad columns [C, ldgx) must be +0"
    return gx[:R, :C]


@pytest.mark.parametrize("C", CS)
def test_log_softmax_bwd_pitches(dev, C):
    """Measured on an MI355X, worst (our error) / (ATen's float32 _log_softmax_backward_data error) per C:
        C        2     3     4     5     13    16    50    63    64      (C = 1: both exact)
        ratio    1.00  1.36  1.16  1.24  1.22  1.26  1.27  1.53  2.73
    (with the row sum as ONE running sum, as the kernel first had it: 1.66 at C = 5, 2.70 at 50, 3.37 at 64, and 5.7 on the
    equal-signed gradient of test_log_softmax_rows_in_autograd_graphs[1000-50-transposed_times_v], which failed its bound.)"""
    worst = 0.0
    for R in RS:
        x = _logits("randn", R, C, dev)
        out = torch.log_softmax(x, -1)                                   # float32 log-probabilities, as the forward hands them on
        g = torch.randn(R, C, device=dev, generator=_gen(77 * C + R % 991, dev))
        g[R // 2] = 0                                                    # a row without gradient
        ref = g.double() - torch.exp(out.double()) * g.double().sum(-1, keepdim=True)
        aten = _err(torch.ops.aten._log_softmax_backward_data(g, out, 1, torch.float32), ref)
        tol = max(4 * aten, 8 * U32 * max(1.0, float(g.abs().max()), float(ref.abs().max())))
        for ldg, ldo in ((C, C), (C + 5, C + 3)):
            for ldgx in sorted({r4(C), min(64, r4(C) + 4)}):
                mine = _err(_run_bwd(g, out, C, ldg, ldo, ldgx), ref)
                print("bwd C=%d R=%d ldg=%d ldgx=%d: ours %.3g aten %.3g tol %.3g" % (C, R, ldg, ldgx, mine, aten, tol))
                assert mine <= tol, (R, ldg, ldgx, mine, aten, tol)
                if aten > 0:
                    worst = max(worst, mine / aten)
    print("bwd C=%d ratio %.2f" % (C, worst))


def test_log_softmax_refuses_short_pitches(dev):
    """The argument checks the wrapper relies on: a gradient pitch below C (0: a row-broadcast gradient) is refused, not read."""
    lib, st = lib_st()
    t = torch.zeros(8, 16, device=dev)
    for ldg in (0, 4):
        assert lib.pn2_log_softmax_bwd(t.data_ptr(), ldg, t.data_ptr(), 8, 8, 5, t.data_ptr(), 8, st) != 0
    assert lib.pn2_log_softmax_fwd(t.data_ptr(), 4, 8, 5, t.data_ptr(), 8, st) != 0          # ldx < round4(C)
    assert lib.pn2_log_softmax_fwd(t.data_ptr(), 8, 8, 5, t.data_ptr(), 4, st) != 0          # ldo < C
    assert lib.pn2_log_softmax_fwd(t.data_ptr(), 68, 8, 65, t.data_ptr(), 65, st) != 0       # C > 64


# ------------------------------------------------------------------------------------------------------ through the wrapper

GRAPHS = {
    "sum": lambda y, a: y.sum(),
    "first_three_columns": lambda y, a: y[:, :3].sum(),
    "transposed_times_v": lambda y, a: (y.t() * a["v"].to(y.dtype)).sum(),
    "column_sums_times_w": lambda y, a: (y.sum(0) * a["w"].to(y.dtype)).sum(),      # a row-broadcast gradient: pitch 0
    "nll_loss": None,
}


@pytest.mark.parametrize("graph", sorted(GRAPHS))
@pytest.mark.parametrize("P,C", [(257, 13), (1000, 50), (300, 3), (64, 65)])
def test_log_softmax_rows_in_autograd_graphs(dev, graph, P, C):
    """log_softmax_rows(x, C) followed by the graph, value and d/dx against the same graph on F.log_softmax(x[:, :C].double());
    the bound is the module's rule, with ATen's float32 evaluation of the same graph as the yardstick.  C = 65 takes the
    ATen fall-back of the wrapper and must agree all the same."""
    g = _gen(P + C, dev)
    x0 = torch.randn(P, r4(C), device=dev, generator=g) * 3
    aux = {"v": torch.randn(P, device=dev, generator=g), "w": torch.randn(C, device=dev, generator=g)}
    tgt = torch.randint(0, C, (P,), device=dev, generator=g)

    def run(kind):
        x = (x0.double() if kind == "f64" else x0.clone()).requires_grad_(True)
        if kind == "mine":
            y = U.log_softmax_rows(x, C)
        else:
            y = F.log_softmax(x[:, :C], dim=-1)
        if graph == "nll_loss":
            val = nll_loss(y, tgt) if kind == "mine" else F.nll_loss(y, tgt)
        else:
            val = GRAPHS[graph](y, aux)
        val.backward()
        return val.detach().double(), x.grad.double(), y.detach()

    ref, gref, y64 = run("f64")
    aten, gaten, _ = run("aten")
    mine, gmine, _ = run("mine")
    # the value: a float32 sum of P*C (or P) terms; A = the sum of their absolute values
    if graph == "nll_loss":
        A = float(ref.abs())
    else:
        A = float(GRAPHS[graph](y64.abs(), {k: v.abs() for k, v in aux.items()}))
    assert abs(float(mine - ref)) <= max(4 * abs(float(aten - ref)), 8 * U32 * max(1.0, A)), (float(mine), float(ref), float(aten))
    assert bool((gmine[:, C:] == 0).all())
    err, err_aten = float((gmine - gref).abs().max()), float((gaten - gref).abs().max())
    print("%s P=%d C=%d: d/dx ours %.3g aten %.3g" % (graph, P, C, err, err_aten))
    assert err <= max(4 * err_aten, 8 * U32 * max(1.0, float(gref.abs().max()))), (err, err_aten)


# -------------------------------------------------------------------------------------------------- NLL loss through the ABI

def _nll(logp, ld, tgt, w, ignore, grad=0.75, ws=None):
    """pn2_nll_loss_fwd + _bwd on logp [R, C] laid out at pitch ld (pad columns +1e30) -> (loss, denom, dlogp [R, ld])."""
    lib, st = lib_st()
    R, C = logp.shape
    dev = logp.device
    lp = torch.full((R, ld), 1e30, device=dev)
    lp[:, :C] = logp
    if ws is None:
        ws = torch.zeros(int(lib.pn2_nll_loss_workspace_bytes(R)), dtype=torch.uint8, device=dev)
    res = sentinel((2,), dev)
    assert lib.pn2_nll_loss_fwd(lp.data_ptr(), ld, tgt.data_ptr(), _lib.ptr(w), R, C, ignore, ws.data_ptr(), res.data_ptr(),
                                res.data_ptr() + 4, st) == 0
    gl = torch.full((1,), grad, device=dev)
    d = sentinel((R + 1, ld), dev)
    assert lib.pn2_nll_loss_bwd(tgt.data_ptr(), _lib.ptr(w), R, C, ignore, gl.data_ptr(), res.data_ptr() + 4, d.data_ptr(), ld, st) == 0
    assert bool(is_sent(d[R]).all()), "wrote past its R rows"
    return res[0], res[1], d[:R]


NLL_RS = (1, 7, 262144 + 257)                       # the last: one row past the 1024 x 256 grid, the grid-stride loop runs twice
WEIGHTS = ("none", "weighted", "zeros")
IGNORES = (-100, "first", "last")


@pytest.mark.parametrize("C", [1, 5, 13, 50])
@pytest.mark.parametrize("R", NLL_RS)
def test_nll_loss_abi_pitches_weights_and_ignore(dev, R, C):
    g = torch.Generator().manual_seed(R + C)
    lp = torch.log_softmax(torch.randn(R, C, generator=g) * 3, dim=-1)
    lp_dev = lp.to(dev)
    for wi, wkind in enumerate(WEIGHTS):
        # every (weight kind, ignore_index) pair appears at some (R, C); each (R, C) sees all weight kinds and all ignore values
        ign = IGNORES[(wi + NLL_RS.index(R) + C) % 3]
        ignore = {"first": 0, "last": C - 1}.get(ign, ign)
        tgt = torch.randint(0, C, (R,), generator=g)
        if ignore == -100:
            tgt[::3] = -100
        w = None if wkind == "none" else torch.rand(C, generator=g) + 0.5
        if wkind == "zeros":
            w[1::2] = 0
            if C > 2:
                tgt[R - 1] = 2                                   # at least one row that counts: a weight sum of 0 is not the subject
        ref_in = lp.double().requires_grad_(True)
        ref = F.nll_loss(ref_in, tgt, weight=None if w is None else w.double(), ignore_index=ignore)
        (ref * 0.75).backward()
        dref = ref_in.grad.float()
        for ld in (C, r4(C) + 4):
            loss, denom, d = _nll(lp_dev, ld, tgt.to(dev), None if w is None else w.to(dev), ignore)
            what = (wkind, ign, ld)
            if bool(torch.isnan(ref)):                           # every row ignored (C = 1 with ignore_index 0)
                assert bool(torch.isnan(loss)) and bool((d == 0).all()), what
                continue
            assert abs(float(loss) - float(ref)) <= 2e-6 * abs(float(ref)), (what, float(loss), float(ref))
            assert bool((d[:, C:].contiguous().view(I32) == 0).all()), ("pad columns must read 0", what)
            assert float((d[:, :C].cpu() - dref).abs().max()) <= 1e-6 * float(dref.abs().max()), what


@pytest.mark.parametrize("C,ld", [(5, 5), (5, 12), (13, 20), (50, 56), (1, 8)])
def test_nll_loss_target_out_of_range(dev, C, ld):
    """A target outside [0, C) that is not ignore_index: the loss is NaN and that row of dlogp is all zeros, the pad columns
    included -- a target in [C, ld) used to put its gradient INTO a pad column (and read the weight vector past its end;
    the weights here have ld entries so that no version of the kernel reads outside them)."""
    R = 300
    g = torch.Generator().manual_seed(C + ld)
    lp = torch.log_softmax(torch.randn(R, C, generator=g) * 3, dim=-1).to(dev)
    for bad in (-1, C) + ((ld - 1,) if ld > C else ()):
        for weighted in (False, True):
            tgt = torch.randint(0, C, (R,), generator=g)
            tgt[17] = bad
            w = (torch.rand(ld, generator=g) + 0.5).to(dev) if weighted else None
            loss, denom, d = _nll(lp, ld, tgt.to(dev), w, -100)
            assert bool(torch.isnan(loss)), (bad, weighted)
            assert bool((d[17].view(I32) == 0).all()), (bad, weighted, d[17])
            assert bool((d[:, C:].contiguous().view(I32) == 0).all()), (bad, weighted)
            assert int((d[:, :C] != 0).sum()) == R - 1           # the other rows keep their one entry


def test_nll_loss_all_rows_ignored(dev):
    lp = torch.log_softmax(torch.randn(600, 7), dim=-1).to(dev)
    for ld in (7, 12):
        for ignore, t in ((-100, -100), (3, 3)):
            loss, denom, d = _nll(lp, ld, torch.full((600,), t, device=dev), None, ignore)
            assert bool(torch.isnan(loss)) and float(denom) == 0.0
            assert bool((d.contiguous().view(I32) == 0).all())


def test_nll_loss_ticket_resets_itself(dev):
    """Two launches back to back on one workspace, then one launch captured in a graph and replayed three times: the same
    loss bits every time (the last workgroup hands the ticket back at 0)."""
    lib, st = lib_st()
    R, C = 70001, 13
    g = torch.Generator().manual_seed(5)
    lp = torch.log_softmax(torch.randn(R, C, generator=g) * 3, dim=-1).to(dev)
    tgt = torch.randint(0, C, (R,), generator=g).to(dev)
    w = (torch.rand(C, generator=g) + 0.5).to(dev)
    ws = torch.zeros(int(lib.pn2_nll_loss_workspace_bytes(R)), dtype=torch.uint8, device=dev)
    first = _nll(lp, C, tgt, w, -100, ws=ws)[0].clone()
    second = _nll(lp, C, tgt, w, -100, ws=ws)[0].clone()
    assert first.view(I32).item() == second.view(I32).item() and bool(torch.isfinite(first))
    res = sentinel((2,), dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = lib.pn2_nll_loss_fwd(lp.data_ptr(), C, tgt.data_ptr(), w.data_ptr(), R, C, -100, ws.data_ptr(), res.data_ptr(),
                                  res.data_ptr() + 4, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    for _ in range(3):
        res.copy_(sentinel((2,), dev))
        graph.replay()
        torch.cuda.synchronize()
        assert res[0].view(I32).item() == first.view(I32).item()
