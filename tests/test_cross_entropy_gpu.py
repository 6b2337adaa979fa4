"""GPU: pn2_cross_entropy_fwd / _bwd (csrc/loss.hip; the criterion of pcdseg.py:178-179) through the C ABI and through
loss.cross_entropy / CrossEntropyLoss, against F.cross_entropy on float64 CPU copies of the same float32 inputs (gradients by
autograd on those copies).

TOLERANCE: the rule of tests/test_loss_tail_gpu.py, per case
    max(4 x the error of ATen's float32 F.cross_entropy on the same device against the same fp64 answer,  8 * 2^-24 * max(1, M)),
M = the largest finite |l_r| for reduction "none", |result| for a reduced loss, the largest gradient entry for the gradient.
ATen on the GPU is only ever given valid targets (it device-asserts on others).

Every output buffer is pre-filled with a NaN pattern no kernel produces and has a spare row: what a kernel promises to write
must be written; pad columns and the spare row must still hold the pattern.

The ratios quoted in the docstrings below were measured with an earlier draw of the options (every second class of zero weight,
"ignore_0" targets drawn from 0 .. C - 1); make_option() has since been changed to keep the share of trivial rows near a quarter,
and the figures have not been re-measured with the present draw.
"""
import pytest
import torch
import torch.nn.functional as F

from pointnet12_amd import _lib
from pointnet12_amd.loss import CrossEntropyLoss, cross_entropy

pytestmark = pytest.mark.gpu

SENT = 0x7FC0DEAD                        # a quiet-NaN bit pattern no kernel produces
I32 = torch.int32
U32 = 2.0 ** -24
CS = (1, 2, 3, 4, 5, 13, 19, 50, 63, 64)
RS = (1, 63, 64, 65, 255, 256, 257)
R_BIG = 262145                           # one row past the forward's 1024 x 256 grid: its grid-stride loop runs twice
BNS = ((1, 1), (3, 7), (2, 64), (2, 100))
KINDS = ("randn", "shifted", "neg_inf_off_target", "neg_inf_at_target", "all_equal", "log_softmaxed")
OPTIONS = ("plain", "weights", "zero_weights", "ignore_m100", "ignore_0")
REDUCTIONS = ("none", "mean", "sum")
EPS = (0.0, 0.1)
RED_ID = {"none": 0, "mean": 1, "sum": 2}


def r4(c):
    return (c + 3) & ~3


def pitches(C):
    return (C, r4(C), r4(C) + 4, C + 3)


def lib_st():
    return _lib.load(), torch.cuda.current_stream().cuda_stream


def sentinel(shape, dev):
    return torch.full(shape, SENT, dtype=I32, device=dev).view(torch.float32)


def is_sent(t):
    return t.contiguous().view(I32) == SENT


def _err(a, ref):
    """max |a - ref| over the finite entries of ref; where ref is infinite a must be the same infinity, where NaN, NaN."""
    a, ref = a.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    fin = torch.isfinite(ref)
    bad_a, bad_r = a[~fin], ref[~fin]
    assert bool((torch.isnan(bad_a) == torch.isnan(bad_r)).all()) and torch.equal(bad_a[~torch.isnan(bad_r)], bad_r[~torch.isnan(bad_r)]), \
        (bad_a, bad_r)
    return float((a - ref)[fin].abs().max()) if bool(fin.any()) else 0.0


def _finite_max(t):
    t = t.detach().double().reshape(-1)
    t = t[torch.isfinite(t)]
    return float(t.abs().max()) if t.numel() else 0.0


# ------------------------------------------------------------------------------------------------------------- inputs (CPU)

def make_option(opt, R, C, g):
    """-> (target [R] int64, weight [C] or None, ignore_index).  The last row always counts: it is neither ignored nor of zero
    weight, so "mean" has a denominator (C = 1 with ignore_index 0 cannot have one: every target is 0; the reference is NaN then
    and the kernel must be too).  At most about a quarter of the rows is ignored or of zero weight where C allows it: every
    fourth class has weight 0 under "zero_weights" (at C = 2 that is one class of two), and under "ignore_0" the targets are
    drawn from 1 .. C - 1 with one row in eight set to the ignored class 0."""
    tgt = torch.randint(0, C, (R,), generator=g)
    w, ignore, live = None, -100, 0
    if opt == "weights":
        w = torch.rand(C, generator=g) + 0.5
    elif opt == "zero_weights":
        w = torch.rand(C, generator=g) + 0.5
        w[1::4] = 0
    elif opt == "ignore_m100":
        tgt[torch.rand(R, generator=g) < 0.25] = -100
    elif opt == "ignore_0":
        ignore, live = 0, min(2, C - 1)
        if C > 1:
            tgt = torch.randint(1, C, (R,), generator=g)
            tgt[torch.rand(R, generator=g) < 0.125] = 0
    tgt[R - 1] = live
    return tgt, w, ignore


def make_rows(kind, R, C, tgt, g):
    """-> x [R, C] float32, or None where the kind does not exist (an off-target column needs C >= 2; -inf at the only column
    is an all -inf row)."""
    x = torch.randn(R, C, generator=g) * 3
    rows = torch.arange(R)
    t = tgt.clamp(0, C - 1)
    if kind == "shifted":
        x = x + torch.where(rows % 2 == 0, 1e4, -1e4)[:, None]
    elif kind == "neg_inf_off_target":
        if C < 2:
            return None
        x[rows, (t + 1 + torch.randint(0, C - 1, (R,), generator=g)) % C] = float("-inf")
    elif kind == "neg_inf_at_target":
        if C < 2:
            return None
        hit = rows % 3 == 0
        x[rows[hit], t[hit]] = float("-inf")
    elif kind == "all_equal":
        x[0] = 2.5
        x[R // 2] = -7.0
    elif kind == "log_softmaxed":
        x = torch.log_softmax(x, -1)                           # the reference's actual input: lse = 0 up to rounding
    return x


def reference(x, tgt, w, ignore, red, eps, gout, dev):
    """fp64 CPU F.cross_entropy and ATen's float32 one on the device -> ((loss, grad) fp64, (loss, grad) ATen)."""
    out = []
    for kind in ("f64", "aten"):
        xi = (x.double() if kind == "f64" else x.to(dev)).requires_grad_(True)
        wi = None if w is None else (w.double() if kind == "f64" else w.to(dev))
        ti, gi = (tgt, gout.double()) if kind == "f64" else (tgt.to(dev), gout.to(dev))
        loss = F.cross_entropy(xi, ti, weight=wi, ignore_index=ignore, reduction=red, label_smoothing=eps)
        (loss * gi).sum().backward()
        out.append((loss.detach(), xi.grad))
    return out


# ---------------------------------------------------------------------------------------------------------- through the ABI

def run_abi(x, layout, tgt, w, ignore, red, eps, gout, dev, ws=None):
    """pn2_cross_entropy_fwd + _bwd on x [R, C] (CPU) laid out on the device as `layout`: ("rows", ld) with 1e30 in the pad
    columns, or ("bcn", B, N) -> (loss, logsum [R], dx [R, C]); the sentinels are checked here."""
    lib, st = lib_st()
    R, C = x.shape
    if layout[0] == "rows":
        ld, inner = layout[1], 0
        xd = torch.full((R, ld), 1e30, device=dev)
        xd[:, :C] = x.to(dev)
        dx = sentinel((R + 1, ld), dev)
    else:
        _, B, N = layout
        ld, inner = 0, N
        xd = x.to(dev).view(B, N, C).transpose(1, 2).contiguous()
        dx = sentinel((B + 1, C, N), dev)
    td = tgt.to(dev)
    wd = None if w is None else w.to(dev)
    if ws is None:
        ws = torch.zeros(int(lib.pn2_cross_entropy_workspace_bytes(R)), dtype=torch.uint8, device=dev)
    lse = sentinel((R + 1,), dev)
    n_out = R if red == "none" else 2                          # reduced: loss, denom
    out = sentinel((n_out + 1,), dev)
    rid = RED_ID[red]
    assert lib.pn2_cross_entropy_fwd(xd.data_ptr(), ld, inner, td.data_ptr(), _lib.ptr(wd), R, C, ignore, eps, rid,
                                     ws.data_ptr() if rid else None, lse.data_ptr(), out.data_ptr(),
                                     out.data_ptr() + 4 if rid else None, st) == 0
    gd = gout.to(dev).reshape(-1).contiguous()
    assert lib.pn2_cross_entropy_bwd(xd.data_ptr(), ld, inner, td.data_ptr(), _lib.ptr(wd), lse.data_ptr(), R, C, ignore, eps, rid,
                                     gd.data_ptr(), out.data_ptr() + 4 if rid else None, dx.data_ptr(), st) == 0
    assert bool(is_sent(lse[R])) and not bool(is_sent(lse[:R]).any()), "logsum: R values, no more"
    assert bool(is_sent(out[n_out])) and not bool(is_sent(out[:n_out]).any()), "loss: its values, no more"
    if layout[0] == "rows":
        assert bool(is_sent(dx[R]).all()), "wrote past its R rows"
        assert bool(is_sent(dx[:R, C:]).all()), "wrote into the pad columns"
        assert not bool(is_sent(dx[:R, :C]).any()), "left a gradient entry unwritten"
        grad = dx[:R, :C]
    else:
        assert bool(is_sent(dx[B]).all()), "wrote past its B clouds"
        assert not bool(is_sent(dx[:B]).any()), "left a gradient entry unwritten"
        grad = dx[:B].transpose(1, 2).reshape(R, C)
    loss = out[:R] if red == "none" else out[0]
    return loss, lse[:R], grad, (out[1] if rid else None)


def check_case(x, layout, tgt, w, ignore, red, eps, g, dev, worst, what):
    """One (input, layout, option, reduction, eps): forward and backward within the rule; returns nothing, updates worst ratios."""
    R, C = x.shape
    gout = torch.randn(R, generator=g) if red == "none" else torch.tensor(0.75)
    (ref, gref), (aten, gaten) = reference(x, tgt, w, ignore, red, eps, gout, dev)
    loss, lse, grad, denom = run_abi(x, layout, tgt, w, ignore, red, eps, gout, dev)
    live = tgt != ignore
    a_l, a_g = _err(aten, ref), _err(gaten, gref)
    m_l, m_g = _err(loss, ref), _err(grad, gref)
    tol_l = max(4 * a_l, 8 * U32 * max(1.0, _finite_max(ref)))
    tol_g = max(4 * a_g, 8 * U32 * max(1.0, _finite_max(gref)))
    print("%s: loss ours %.3g aten %.3g tol %.3g | grad ours %.3g aten %.3g tol %.3g" % (what, m_l, a_l, tol_l, m_g, a_g, tol_g))
    assert m_l <= tol_l, (what, "loss", m_l, a_l, tol_l)
    assert m_g <= tol_g, (what, "grad", m_g, a_g, tol_g)
    gc = grad.cpu()
    assert bool((gc[~live] == 0).all()), (what, "ignored rows must have a zero gradient")
    if red == "none":
        assert bool((loss.cpu()[~live] == 0).all()), (what, "ignored rows must have a zero loss")
    else:
        dref = float((torch.ones(C) if w is None else w)[tgt[live]].double().sum())
        assert abs(float(denom) - dref) <= 4 * U32 * max(1.0, dref), (what, "denominator")
    minf = torch.isinf(x) & live[:, None]
    if eps == 0.0 and bool(minf.any()):
        off = minf.clone()
        off[torch.arange(R)[live], tgt[live]] = False
        assert bool((gc[off] == 0).all()), (what, "a -inf logit off the target has gradient exactly 0")
    ref_lse = torch.logsumexp((x - x.max(-1, keepdim=True).values).double(), -1)
    assert _err(lse, ref_lse) <= 8 * U32 * max(1.0, _finite_max(ref_lse)), (what, "logsum")
    if a_l > 0:
        worst["loss"] = max(worst["loss"], m_l / a_l)
    if a_g > 0:
        worst["grad"] = max(worst["grad"], m_g / a_g)


def sweep(C, Rs, layouts_of, dev, seed, j0=0):
    """NOT a full cross of kind x layout x combination (run time): for every R all 30 (option, reduction, label smoothing)
    combinations, with the row kind and the layout rotating: combination i
    at the j-th R takes kind (i + j) % 6 and layout (i + i // 6 + j) % len(layouts).  Over the 7 R of the row-major sweep (and
    over the 4 (B, N) of the class-strided one, 4 of the 6 kinds) each combination meets every kind and every pitch, and each R
    every kind and every pitch.  Where a kind does not exist (C = 1) the next one that does is taken."""
    worst = {"loss": 0.0, "grad": 0.0}
    for j, R in enumerate(Rs, j0):
        layouts = layouts_of(R)
        i = 0
        for opt in OPTIONS:
            for red in REDUCTIONS:
                for eps in EPS:
                    g = torch.Generator().manual_seed(seed + 7919 * R + i)
                    tgt, w, ignore = make_option(opt, R, C, g)
                    k = (i + j) % len(KINDS)
                    x = make_rows(KINDS[k], R, C, tgt, g)
                    while x is None:
                        k = (k + 1) % len(KINDS)
                        x = make_rows(KINDS[k], R, C, tgt, g)
                    layout = layouts[(i + i // 6 + j) % len(layouts)]
                    i += 1
                    check_case(x, layout, tgt, w, ignore, red, eps, g, dev, worst,
                               "C=%d R=%d %s %s %s eps=%g %s" % (C, R, KINDS[k], opt, red, eps, layout))
    return worst


@pytest.mark.parametrize("C", CS)
def test_abi_row_major_sweep(dev, C):
    """R in 1, 63, 64, 65, 255, 256, 257 x option x reduction x label smoothing; each of those cases takes ONE row kind and ONE
    pitch (C, round4(C), round4(C) + 4, C + 3; 1e30 in the pad columns), rotating as sweep() says: a covering, not a full cross.

    Measured on an MI355X, worst (our error) / (ATen's float32 error) per C over the cases in which ATen is not exact:
        C        2      3     4      5     13     19    50     63     64       (C = 1: both exact)
        loss     3.68   1.43  2.93   2.46  15.60  2.26  2.15   1.58   1.28
        grad     17.61  2.08  15.50  4.94  9.36   2.60  16.69  34.27  6.08
    Every ratio above 4 is a single row (R = 1) on which ATen happens to err by 1e-8 or less and the kernel by 1e-7 .. 4e-7: the
    floor of the rule, 4.8e-7, admits those.  The case nearest its bound: C = 63, R = 256, "none", eps 0.1, gradient error
    1.15e-6 against 3.4e-7 for ATen, bound 1.87e-6.
    """
    worst = sweep(C, RS, lambda R: [("rows", ld) for ld in pitches(C)], dev, 1000 * C)
    print("rows C=%d ratio loss %.2f grad %.2f" % (C, worst["loss"], worst["grad"]))


@pytest.mark.parametrize("C", CS)
def test_abi_class_strided_sweep(dev, C):
    """The [B, C, N] layout, (B, N) in (1, 1), (3, 7), (2, 64), (2, 100) x option x reduction x smoothing, the row kind rotating (each
    combination meets 4 of the 6 kinds here).

    Measured on an MI355X, worst (our error) / (ATen's float32 error) per C:
        C        2     3     4      5     13    19    50    63     64       (C = 1: both exact)
        loss     3.07  1.18  13.17  3.31  9.75  1.75  1.78  9.52   1.24
        grad     2.53  2.31  16.38  5.32  6.81  3.03  3.56  13.33  3.74
    (the ratios above 4 again at (B, N) = (1, 1), under the floor of the rule).  The case nearest its bound: C = 63, (3, 7), "none",
    eps 0.1, one -inf per row: gradient error 7.0e-7 against 2.3e-7 for ATen, bound 1.02e-6.
    """
    worst = {"loss": 0.0, "grad": 0.0}
    for j, (B, N) in enumerate(BNS):
        w = sweep(C, (B * N,), lambda R: [("bcn", B, N)], dev, 1000 * C + 17, j0=j)
        worst = {k: max(worst[k], w[k]) for k in worst}
    print("bcn C=%d ratio loss %.2f grad %.2f" % (C, worst["loss"], worst["grad"]))


def test_abi_grid_stride_loop(dev):
    """R = 262 145, C = 3: one row more than 1024 workgroups of 256 take in one pass.  Every option x reduction x smoothing once,
    the kind and the layout (four pitches and [5, 3, 52429]) rotating.  Measured: worst ratio 1.04 (loss), 1.44 (gradient)."""
    C, R = 3, R_BIG
    layouts = [("rows", ld) for ld in pitches(C)] + [("bcn", 5, R // 5)]
    worst = {"loss": 0.0, "grad": 0.0}
    n = 0
    for oi, opt in enumerate(OPTIONS):
        for red in REDUCTIONS:
            for eps in EPS:
                g = torch.Generator().manual_seed(31 + n)
                tgt, w, ignore = make_option(opt, R, C, g)
                kind = KINDS[n % len(KINDS)]
                x = make_rows(kind, R, C, tgt, g)
                check_case(x, layouts[n % len(layouts)], tgt, w, ignore, red, eps, g, dev, worst,
                           "R=%d %s %s %s eps=%g %s" % (R, kind, opt, red, eps, layouts[n % len(layouts)]))
                n += 1
    print("big R ratio loss %.2f grad %.2f" % (worst["loss"], worst["grad"]))


# ----------------------------------------------------------------------------------------------------------- dedicated cases

@pytest.mark.parametrize("layout", [("rows", 7), ("rows", 12), ("bcn", 3, 200)], ids=str)
def test_all_rows_ignored(dev, layout):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(600, 7, generator=g) * 3
    for ignore, t in ((-100, -100), (3, 3)):
        tgt = torch.full((600,), t)
        for eps in EPS:
            loss, _, grad, denom = run_abi(x, layout, tgt, None, ignore, "mean", eps, torch.tensor(1.0), dev)
            assert bool(torch.isnan(loss)) and float(denom) == 0.0 and bool((grad == 0).all())
            loss, _, grad, denom = run_abi(x, layout, tgt, None, ignore, "sum", eps, torch.tensor(1.0), dev)
            assert float(loss) == 0.0 and bool((grad == 0).all())
            loss, _, grad, _ = run_abi(x, layout, tgt, None, ignore, "none", eps, torch.ones(600), dev)
            assert bool((loss == 0).all()) and bool((grad == 0).all())


def test_every_live_target_in_a_zero_weight_class(dev):
    """The sum of the weights is 0: "mean" is NaN, as torch on the CPU; "sum" is what torch says."""
    g = torch.Generator().manual_seed(4)
    R, C = 300, 5
    x = torch.randn(R, C, generator=g) * 3
    w = torch.tensor([0.7, 0.0, 1.3, 0.0, 0.9])
    tgt = torch.randint(0, 2, (R,), generator=g) * 2 + 1            # classes 1 and 3
    tgt[::4] = -100
    for eps in EPS:
        ref = F.cross_entropy(x.double(), tgt, weight=w.double(), reduction="mean", label_smoothing=eps)
        loss, _, _, denom = run_abi(x, ("rows", 8), tgt, w, -100, "mean", eps, torch.tensor(1.0), dev)
        assert bool(torch.isnan(ref)) and bool(torch.isnan(loss)) and float(denom) == 0.0
        ref = F.cross_entropy(x.double(), tgt, weight=w.double(), reduction="sum", label_smoothing=eps)
        loss, _, _, _ = run_abi(x, ("rows", 8), tgt, w, -100, "sum", eps, torch.tensor(1.0), dev)
        assert _err(loss, ref) <= 8 * U32 * max(1.0, float(ref.abs()))


@pytest.mark.parametrize("layout", [("rows", 1), ("rows", 4), ("rows", 8), ("bcn", 2, 150)], ids=str)
def test_one_class_is_loss_zero_gradient_zero(dev, layout):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(300, 1, generator=g) * 30
    tgt = torch.zeros(300, dtype=torch.int64)
    for red in REDUCTIONS:
        for eps in EPS:
            gout = torch.randn(300, generator=g) if red == "none" else torch.tensor(2.0)
            loss, lse, grad, _ = run_abi(x, layout, tgt, None, -100, red, eps, gout, dev)
            assert bool((loss == 0).all()) and bool((grad == 0).all()) and bool((lse == 0).all()), (red, eps)


@pytest.mark.parametrize("C,layout", [(5, ("rows", 5)), (5, ("rows", 12)), (13, ("rows", 16)), (50, ("rows", 53)), (1, ("rows", 8)),
                                      (19, ("bcn", 3, 100))], ids=str)
def test_target_out_of_range(dev, C, layout):
    """Targets C and -1 (never larger: a kernel that indexed with them would stay inside the buffers here) among valid ones,
    given to our kernel only: the reduced loss is NaN, those rows are NaN in "none" and zero in dx, and the other rows' "none"
    values and gradient directions are what they are without the bad rows."""
    R = 300
    g = torch.Generator().manual_seed(C + 100)
    x = torch.randn(R, C, generator=g) * 3
    w = torch.rand(C, generator=g) + 0.5
    bad_rows = torch.tensor([17, 64, 255, 299])
    for bad in (C, -1):
        for weight in (None, w):
            for eps in EPS:
                tgt = torch.randint(0, C, (R,), generator=g)
                good = tgt.clone()
                good[bad_rows] = -100                                 # the same problem with the bad rows ignored instead
                tgt[bad_rows] = bad
                gout = torch.randn(R, generator=g)
                what = (bad, weight is not None, eps)
                loss, _, grad, _ = run_abi(x, layout, tgt, weight, -100, "none", eps, gout, dev)
                want, _, gwant, _ = run_abi(x, layout, good, weight, -100, "none", eps, gout, dev)
                keep = torch.ones(R, dtype=torch.bool)
                keep[bad_rows] = False
                assert bool(torch.isnan(loss.cpu()[bad_rows]).all()) and bool((grad.cpu()[bad_rows] == 0).all()), what
                assert torch.equal(loss.cpu()[keep], want.cpu()[keep]) and torch.equal(grad.cpu()[keep], gwant.cpu()[keep]), what
                assert bool(torch.isfinite(want).all())
                ref = F.cross_entropy(x.double(), good, weight=None if weight is None else weight.double(), reduction="none",
                                      label_smoothing=eps)
                assert _err(want, ref) <= 8 * U32 * max(1.0, float(ref.abs().max())), what
                for red in ("mean", "sum"):
                    loss, _, grad, denom = run_abi(x, layout, tgt, weight, -100, red, eps, torch.tensor(1.0), dev)
                    _, _, gwant, dwant = run_abi(x, layout, good, weight, -100, red, eps, torch.tensor(1.0), dev)
                    assert bool(torch.isnan(loss)) and bool((grad.cpu()[bad_rows] == 0).all()), (what, red)
                    assert float(denom) == float(dwant) and torch.equal(grad.cpu()[keep], gwant.cpu()[keep]), (what, red)


def test_ticket_resets_itself(dev):
    """Two reduced forwards on ONE workspace with no memset in between, with different grids (2 and 274 workgroups), then the
    first again: each is right, and the repeat has the first one's bits."""
    lib, _ = lib_st()
    g = torch.Generator().manual_seed(6)
    C = 13
    ws = torch.zeros(int(lib.pn2_cross_entropy_workspace_bytes(70001)), dtype=torch.uint8, device=dev)
    w = torch.rand(C, generator=g) + 0.5
    got = []
    for R in (300, 70001, 300):
        gr = torch.Generator().manual_seed(R)
        x = torch.randn(R, C, generator=gr) * 3
        tgt = torch.randint(0, C, (R,), generator=gr)
        ref = F.cross_entropy(x.double(), tgt, weight=w.double(), label_smoothing=0.1)
        loss, _, _, _ = run_abi(x, ("rows", 16), tgt, w, -100, "mean", 0.1, torch.tensor(1.0), dev, ws=ws)
        assert _err(loss, ref) <= 8 * U32 * max(1.0, float(ref.abs())), R
        got.append(loss.view(I32).item())
    assert got[0] == got[2]
    assert int(ws.view(I32)[-4]) == 0                            # the ticket is back at 0


# ---------------------------------------------------------------------------------------------------- through the Python API

def _rule(mine, aten, ref):
    e, a = _err(mine, ref), _err(aten, ref)
    assert e <= max(4 * a, 8 * U32 * max(1.0, _finite_max(ref))), (e, a)


def test_pcdseg_form_transposed_view_of_the_model_output(dev):
    """CrossEntropyLoss()(logp.transpose(2, 1), target) on a [2, 257, 19] leaf of log-probabilities (pcdseg.py:178-179): value and
    logp.grad within the rule, logp.grad contiguous [B, N, C], and no [R, C] copy of the input anywhere."""
    B, N, C = 2, 257, 19
    g = torch.Generator().manual_seed(7)
    lp0 = torch.log_softmax(torch.randn(B, N, C, generator=g) * 3, -1)
    tgt = torch.randint(0, C, (B, N), generator=g)
    ref_in = lp0.double().requires_grad_(True)
    ref = torch.nn.CrossEntropyLoss()(ref_in.transpose(2, 1), tgt)
    ref.backward()
    at_in = lp0.to(dev).requires_grad_(True)
    aten = torch.nn.CrossEntropyLoss()(at_in.transpose(2, 1), tgt.to(dev))
    aten.backward()
    td = tgt.to(dev)
    crit = CrossEntropyLoss()
    forward_bytes = []
    for _ in range(2):          # (the first call may be the one that allocates the 16 MiB zero arena the workspace comes from)
        logp = lp0.to(dev).requires_grad_(True)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(dev)
        loss = crit(logp.transpose(2, 1), td)
        forward_bytes.append(torch.cuda.memory_allocated(dev) - before)
    assert min(forward_bytes) < B * N * C * 4, forward_bytes                     # logsum [R] and two scalars, no [R, C] tensor
    saved = loss.grad_fn.saved_tensors[0]
    assert saved.untyped_storage().data_ptr() == logp.untyped_storage().data_ptr() and saved.stride() == (N * C, 1, C)
    loss.backward()
    backward_bytes = torch.cuda.memory_allocated(dev) - before
    assert backward_bytes < 2 * B * N * C * 4, backward_bytes                    # the gradient itself and nothing of its size beside it
    assert logp.grad.shape == (B, N, C) and logp.grad.is_contiguous()
    _rule(loss, aten, ref)
    _rule(logp.grad, at_in.grad, ref_in.grad)


def test_column_slice_of_a_padded_buffer_and_contiguous_bcn(dev):
    """[R, C] as log_softmax_rows' producer hands it over (the C leading columns of [R, round4(C)]), and contiguous [B, C, N]."""
    g = torch.Generator().manual_seed(8)
    R, C = 257, 13
    w = torch.rand(C, generator=g) + 0.5
    tgt = torch.randint(0, C, (R,), generator=g)
    tgt[::5] = -100
    buf0 = torch.randn(R, r4(C), generator=g) * 3
    kw = dict(ignore_index=-100, label_smoothing=0.1)
    ref_in = buf0.double().requires_grad_(True)
    ref = F.cross_entropy(ref_in[:, :C], tgt, weight=w.double(), **kw)
    ref.backward()
    at_in = buf0.to(dev).requires_grad_(True)
    aten = F.cross_entropy(at_in[:, :C], tgt.to(dev), weight=w.to(dev), **kw)
    aten.backward()
    buf = buf0.to(dev).requires_grad_(True)
    loss = cross_entropy(buf[:, :C], tgt.to(dev), weight=w.to(dev), **kw)
    assert loss.grad_fn.saved_tensors[0].stride() == (r4(C), 1)
    loss.backward()
    _rule(loss, aten, ref)
    _rule(buf.grad, at_in.grad, ref_in.grad)
    assert bool((buf.grad[:, C:] == 0).all())
    # [B, C, N] contiguous, a [B, N] target, reduction "sum"
    B, N = 3, 100
    x0 = torch.randn(B, C, N, generator=g) * 3
    t2 = torch.randint(0, C, (B, N), generator=g)
    ref_in = x0.double().requires_grad_(True)
    ref = F.cross_entropy(ref_in, t2, reduction="sum")
    ref.backward()
    at_in = x0.to(dev).requires_grad_(True)
    aten = F.cross_entropy(at_in, t2.to(dev), reduction="sum")
    aten.backward()
    xin = x0.to(dev).requires_grad_(True)
    loss = cross_entropy(xin, t2.to(dev), reduction="sum")
    loss.backward()
    _rule(loss, aten, ref)
    _rule(xin.grad, at_in.grad, ref_in.grad)
    with pytest.raises(_lib.Pn2Error):
        cross_entropy(x0.to(dev)[:, :, ::2], t2.to(dev)[:, ::2])                # neither layout: refused, not copied


def _once(x0, tgt, w, dev):
    x = x0.clone().requires_grad_(True)
    loss = cross_entropy(x.transpose(2, 1), tgt, weight=w, label_smoothing=0.1)
    lse = loss.grad_fn.saved_tensors[3].clone()
    loss.backward()
    return loss.detach().clone(), lse, x.grad.clone()


def test_repeat_is_bit_identical(dev):
    g = torch.Generator().manual_seed(9)
    B, N, C = 4, 20000, 19                                        # 313 workgroups: the order they finish in varies
    x0 = (torch.randn(B, N, C, generator=g) * 3).to(dev)
    tgt = torch.randint(0, C, (B, N), generator=g).to(dev)
    w = (torch.rand(C, generator=g) + 0.5).to(dev)
    a, b = _once(x0, tgt, w, dev), _once(x0, tgt, w, dev)
    for u, v in zip(a, b):
        assert torch.equal(u.view(I32), v.view(I32))


def test_forward_and_backward_capture_into_a_graph(dev):
    """Forward + backward captured with torch.cuda.graph at R = 257, C = 19 on static buffers; replayed on fresh data copied
    into them, loss and gradient equal the eager ones bit for bit."""
    g = torch.Generator().manual_seed(10)
    R, C = 257, 19
    sx = (torch.randn(R, C, generator=g) * 3).to(dev).requires_grad_(True)
    st = torch.randint(0, C, (R,), generator=g).to(dev)
    crit = CrossEntropyLoss(label_smoothing=0.1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):                                       # warm-up on the capture stream
            sx.grad = None
            crit(sx, st).backward()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    sx.grad = None
    with torch.cuda.graph(graph):
        sloss = crit(sx, st)
        sloss.backward()
    for seed in (11, 12):
        gg = torch.Generator().manual_seed(seed)
        nx = (torch.randn(R, C, generator=gg) * 3).to(dev)
        nt = torch.randint(0, C, (R,), generator=gg).to(dev)
        nt[::7] = -100
        with torch.no_grad():
            sx.copy_(nx)
            st.copy_(nt)
        graph.replay()
        torch.cuda.synchronize()
        ex = nx.clone().requires_grad_(True)
        eloss = crit(ex, nt)
        eloss.backward()
        assert torch.equal(sloss.detach().view(I32), eloss.detach().view(I32))
        assert torch.equal(sx.grad.view(I32), ex.grad.view(I32))
        ref = F.cross_entropy(nx.double().cpu(), nt.cpu(), label_smoothing=0.1)
        assert _err(sloss, ref) <= 8 * U32 * max(1.0, float(ref.abs()))


def test_upstream_gradients_are_read_on_the_device(dev):
    """"none" under a random upstream vector, "mean" under an upstream scalar other than 1 that lives on the device."""
    g = torch.Generator().manual_seed(13)
    B, N, C = 2, 100, 13
    x0 = torch.randn(B, C, N, generator=g) * 3
    tgt = torch.randint(0, C, (B, N), generator=g)
    tgt[0, ::3] = -100
    v = torch.randn(B, N, generator=g)
    s = torch.tensor(-2.5)
    for red, up in (("none", v), ("mean", s)):
        outs = []
        for kind in ("f64", "aten", "mine"):
            x = (x0.double() if kind == "f64" else x0.to(dev)).requires_grad_(True)
            t, u = (tgt, up.double()) if kind == "f64" else (tgt.to(dev), up.to(dev))
            f = cross_entropy if kind == "mine" else F.cross_entropy
            loss = f(x, t, reduction=red, label_smoothing=0.1)
            assert loss.shape == (() if red == "mean" else (B, N))
            (loss * u).sum().backward()
            outs.append((loss.detach(), x.grad))
        (ref, gref), (aten, gaten), (mine, gmine) = outs
        _rule(mine, aten, ref)
        _rule(gmine, gaten, gref)
        assert gmine.shape == (B, C, N) and gmine.is_contiguous()
