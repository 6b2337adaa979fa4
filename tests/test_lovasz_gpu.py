"""GPU: pn2_lovasz_fwd / pn2_lovasz_bwd (csrc/lovasz.hip) through the C ABI and through loss.py against the rule of
tests/lovasz_ref.py (the cases are generated there; tests/test_lovasz_cpu.py checks on the CPU what they rely on).

Exact part (from_logits=False, drawn float32 probabilities): dp BIT-EQUAL to float32 of the fp64 rule; loss the float32 nearest the
fp64 value or its neighbour (every term e * c_k is >= 0, so fp64 sums in two orders differ by at most n * 2^-53 relative, far below
2^-24 at these sizes).
Softmax part (from_logits=True): prob within 4 x stock float32 torch's own error against the fp64 softmax (floor 8 * 2^-24: the rule
of tests/test_loss_tail_gpu.py); loss and dp as in the exact part against the rule evaluated on the RETURNED prob; |loss - fp64 rule
on the fp64 softmax| <= max|prob - p64| + 2^-24 (the value is 1-Lipschitz in the sup norm); dx per element within
    1.05 (C + 3) 2^-24 |g| p_c (|dp_c| + sum_j |p_j dp_j|)
of the fp64 Jacobian applied to the kernel's own prob and dp.  Counted from the roundings of dx = g * (p_c * (dp_c - s)), s the
float32 sum of the C float32 products p_j dp_j in class order: each product one rounding and at most C - 1 additions above it (C
roundings on sum_j |p_j dp_j|), the subtraction one (on |dp_c| + |s|), the two multiplications one each; 1.05 for second order.

Every output has sentinel guard words around it, the workspace is NaN-filled and guarded behind."""
import ctypes

import numpy as np
import pytest
import torch

import lovasz_ref as L
from pointnet12_amd import _lib
from pointnet12_amd.loss import LovaszSoftmax, lovasz_softmax

pytestmark = pytest.mark.gpu

SENT = 0x7FC0DEAD                        # a quiet-NaN bit pattern no kernel produces
GUARD = 64                               # guard words either side of an output
U24 = 2.0 ** -24


def _tile():
    return int(_lib.load().pn2_lovasz_tile_rows())


def _guarded(n, dev):
    """-> (whole buffer, the n float32 words in its middle); everything holds the sentinel."""
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.int32, device=dev)
    return buf, buf[GUARD:GUARD + n].view(torch.float32)


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all())


def _mask(classes, C, dev):
    if isinstance(classes, str):
        return None
    m = torch.zeros(C, dtype=torch.int32)
    m[list(classes)] = 1
    return m.to(dev)


def run_fwd(x, ld, inner, target, R, C, images, classes, from_logits, want_prob=True):
    """pn2_lovasz_fwd on device memory x -> (rc, loss float32, dp [R, C], prob [R, C] or None), guards checked."""
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    dev = x.device
    nbytes = int(lib.pn2_lovasz_workspace_bytes(R, C, images))
    assert nbytes > 0 and nbytes % 16 == 0
    wsbuf = torch.full((nbytes // 4 + GUARD,), SENT, dtype=torch.int32, device=dev)
    dpb, dp = _guarded(R * C, dev)
    pb, prob = _guarded(R * C, dev)
    lb, loss = _guarded(1, dev)
    mask = _mask(classes, C, dev)
    rc = lib.pn2_lovasz_fwd(x.data_ptr(), ld, inner, target.data_ptr(), R, C, images, L.IGNORE, int(from_logits), _lib.ptr(mask),
                            int(classes == "present"), wsbuf.data_ptr(), dp.data_ptr(), prob.data_ptr() if want_prob else None,
                            loss.data_ptr(), st)
    torch.cuda.synchronize()
    assert _guards_intact(dpb) and _guards_intact(pb) and _guards_intact(lb) and bool((wsbuf[-GUARD:] == SENT).all())
    if not want_prob:
        assert bool((pb == SENT).all())
    return rc, loss.cpu().numpy()[0], dp.view(R, C).cpu().numpy(), prob.view(R, C).cpu().numpy() if want_prob else None


def run_bwd(x, ld, inner, dp, R, C, from_logits, g, dx):
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    gt = torch.tensor([g], dtype=torch.float32, device=x.device)
    rc = lib.pn2_lovasz_bwd(x.data_ptr(), ld, inner, dp.data_ptr(), R, C, int(from_logits), gt.data_ptr(), dx.data_ptr(), st)
    torch.cuda.synchronize()
    return rc


def _check_exact(case, loss, dp, prob=None):
    want_loss, want_dp = L.rule_for(case)
    print(case["name"], "loss", loss, "rule", want_loss)
    if prob is not None:
        assert (prob.view(np.uint32) == case["p"].view(np.uint32)).all(), case["name"]
    assert L.dp_equal(dp, want_dp), (case["name"], int((dp != want_dp.astype(np.float32)).sum()))
    assert L.loss_close(loss, want_loss), (case["name"], loss, want_loss)
    if want_loss == 0.0:
        assert not np.signbit(loss), case["name"]


def test_exact_cases_through_the_c_abi(dev):
    for case in L.exact_cases(_tile()):
        p, t = torch.from_numpy(case["p"]).to(dev), torch.from_numpy(case["target"]).to(dev)
        R, C = case["p"].shape
        rc, loss, dp, prob = run_fwd(p, C, 0, t, R, C, case["images"], case["classes"], False)
        assert rc == 0, case["name"]
        _check_exact(case, loss, dp, prob)
        if "bad_rows" in case:
            assert np.isnan(loss) and not dp[list(case["bad_rows"])].any()
        if case["name"].startswith("ignored_all"):
            assert loss == 0.0 and not np.signbit(loss) and not dp.view(np.uint32).any()


def _layouts(case, dev):
    """name -> (tensor as loss.py takes it, base tensor, ld, inner) of a per-image case in the three layouts."""
    p = torch.from_numpy(case["p"]).to(dev)
    R, C = p.shape
    B = case["images"]
    N = R // B
    ld = C + 5
    padded = torch.full((R, ld), float("nan"), device=dev)
    padded[:, :C] = p
    bnc = p.view(B, N, C).clone()
    bcn = p.view(B, N, C).transpose(1, 2).contiguous()
    return {"padded_pitch": (padded[:, :C], padded, ld, 0), "transposed_bnc": (bnc.transpose(1, 2), bnc, C, 0),
            "contiguous_bcn": (bcn, bcn, 0, N)}


def test_three_layouts_forward_and_backward(dev):
    T = _tile()
    case = {c["name"]: c for c in L.exact_cases(T)}["per_image_present"]
    R, C = case["p"].shape
    B = case["images"]
    want_loss, want_dp = L.rule_for(case)
    t = torch.from_numpy(case["target"]).to(dev)
    g = 0.625
    for name, (view, base, ld, inner) in _layouts(case, dev).items():
        images = 1 if name == "padded_pitch" else B
        ref_case = case if images == B else dict(case, name="per_image_flat", images=1)
        rc, loss, dp, prob = run_fwd(base, ld, inner, t, R, C, images, "present", False)
        assert rc == 0, name
        _check_exact(ref_case, loss, dp, prob)
        # backward through the ABI: g * dp in the input's layout, nothing else touched
        dxb = torch.full((base.numel() + 2 * GUARD,), SENT, dtype=torch.int32, device=dev)
        dx = dxb[GUARD:GUARD + base.numel()].view(torch.float32).view(base.shape)
        assert run_bwd(base, ld, inner, torch.from_numpy(dp).to(dev), R, C, False, g, dx) == 0
        assert _guards_intact(dxb)
        want_dx = (np.float32(g) * dp).astype(np.float32)
        if name == "padded_pitch":
            assert bool((dx[:, C:].contiguous().view(torch.int32) == SENT).all()), "pad columns are never touched"
            got = dx[:, :C].cpu().numpy()
        elif name == "transposed_bnc":
            got = dx.reshape(R, C).cpu().numpy()
        else:
            got = dx.transpose(1, 2).reshape(R, C).cpu().numpy()
        assert (got.view(np.uint32) == want_dx.view(np.uint32)).all(), name
        # and through loss.py: the same loss, the gradient in the input's strides
        leaf = base.clone().requires_grad_(True)
        xv = {"padded_pitch": lambda a: a[:, :C], "transposed_bnc": lambda a: a.transpose(1, 2), "contiguous_bcn": lambda a: a}[name](leaf)
        assert xv.stride() == view.stride()
        seen = []
        xv.register_hook(seen.append)                                     # the gradient as the backward hands it over
        tv = t if name == "padded_pitch" else t.view(B, R // B)
        out = lovasz_softmax(xv, tv, "present", per_image=images == B, ignore_index=L.IGNORE, from_logits=False)
        (out * g).backward()
        assert out.detach().cpu().numpy().view(np.uint32) == np.float32(loss).view(np.uint32), name
        assert seen[0].stride() == xv.stride() and seen[0].shape == xv.shape
        grad = seen[0] if name == "padded_pitch" else seen[0].transpose(1, 2).reshape(R, C)
        assert (grad.cpu().numpy().view(np.uint32) == want_dx.view(np.uint32)).all(), name


def test_softmax_part(dev):
    for case in L.softmax_cases():
        x, t = torch.from_numpy(case["x"]).to(dev), torch.from_numpy(case["target"]).to(dev)
        R, C = case["x"].shape
        rc, loss, dp, prob = run_fwd(x, C, 0, t, R, C, case["images"], case["classes"], True)
        assert rc == 0, case["name"]
        p64 = L.softmax64(case["x"])
        stock = torch.softmax(x, 1).cpu().numpy()
        err, stock_err = np.abs(prob.astype(np.float64) - p64).max(), np.abs(stock.astype(np.float64) - p64).max()
        print(case["name"], "prob err", err, "stock", stock_err)
        assert err <= max(4.0 * stock_err, 8.0 * U24), (case["name"], err, stock_err)
        own = dict(name=case["name"] + "/own_prob", p=prob, target=case["target"], classes=case["classes"], images=case["images"])
        _check_exact(own, loss, dp)
        # the rule on the fp64 softmax itself (errors in fp64): the value is 1-Lipschitz in the sup norm of the errors
        want64 = _rule_on_fp64_probabilities(p64, case["target"], case["classes"], case["images"])
        print(case["name"], "loss", loss, "fp64", want64, "bound", err + U24)
        assert abs(float(loss) - want64) <= err + U24, (case["name"], loss, want64, err)
        # dx against the fp64 Jacobian on the kernel's own prob and dp
        g = -0.7
        dxb, dx = _guarded(R * C, dev)
        assert run_bwd(x, C, 0, torch.from_numpy(dp).to(dev), R, C, True, g, dx) == 0
        assert _guards_intact(dxb)
        P, D = prob.astype(np.float64), dp.astype(np.float64)
        g32 = float(np.float32(g))
        want = g32 * P * (D - (P * D).sum(1, keepdims=True))
        bound = 1.05 * (C + 3) * U24 * abs(g32) * P * (np.abs(D) + np.abs(P * D).sum(1, keepdims=True))
        diff = np.abs(dx.view(R, C).cpu().numpy().astype(np.float64) - want)
        with np.errstate(invalid="ignore", divide="ignore"):
            print(case["name"], "dx worst ratio to bound", np.nanmax(np.where(bound > 0, diff / bound, 0.0)))
        assert (diff <= bound).all(), (case["name"], float((diff - bound).max()))


def _rule_on_fp64_probabilities(p64, target, classes, images):
    """The rule with the errors |fg - p| taken in fp64 (nothing rounded to float32): the yardstick of the Lipschitz check."""
    R, C = p64.shape
    N = R // images
    total = 0.0
    for b in range(images):
        rows = np.arange(b * N, (b + 1) * N)
        rows = rows[target[rows] != L.IGNORE]
        losses = []
        for c in range(C):
            fg = target[rows] == c
            if not (classes == "all" or (classes == "present" and fg.any()) or (not isinstance(classes, str) and c in classes)):
                continue
            e = np.abs(fg.astype(np.float64) - p64[rows, c])
            order = np.lexsort((np.arange(e.size), -e))
            F = np.cumsum(fg[order].astype(np.int64))
            losses.append(float(np.sum(e[order] * L.closed_form(np.arange(1, e.size + 1), F, int(fg.sum())))))
        if losses:
            total += sum(losses) / len(losses)
    return total / images


def test_two_runs_are_byte_identical_and_module_equals_function(dev):
    T = _tile()
    rng = np.random.default_rng(21)
    B, C, N = 3, 19, 2 * T + 7
    x = torch.from_numpy((3 * rng.standard_normal((B, N, C))).astype(np.float32)).to(dev).transpose(1, 2)
    t = torch.from_numpy(L._random_target(rng, B * N, C).reshape(B, N)).to(dev)
    outs = []
    for f in (lambda a, b: lovasz_softmax(a, b, "present", True, L.IGNORE), lambda a, b: lovasz_softmax(a, b, "present", True, L.IGNORE),
              LovaszSoftmax("present", True, L.IGNORE)):
        xv = x.detach().requires_grad_(True)
        loss = f(xv, t)
        loss.backward()
        outs.append((loss.detach().clone(), xv.grad.clone()))
    for loss, grad in outs[1:]:
        assert torch.equal(loss.view(torch.int32), outs[0][0].view(torch.int32)) and torch.equal(grad.view(torch.int32), outs[0][1].view(torch.int32))
    assert bool(torch.isfinite(outs[0][1]).all()) and float(outs[0][0]) > 0
    rcs = [run_fwd(x.transpose(1, 2).contiguous().view(B * N, C), C, 0, t.view(-1), B * N, C, B, "present", True) for _ in range(2)]
    assert rcs[0][1].view(np.uint32) == rcs[1][1].view(np.uint32) and (rcs[0][2].view(np.uint32) == rcs[1][2].view(np.uint32)).all()
    assert rcs[0][1].view(np.uint32) == outs[0][0].cpu().numpy().view(np.uint32)


def test_captured_forward_and_backward_replays_bit_for_bit(dev):
    T = _tile()
    rng = np.random.default_rng(22)
    B, C, N = 2, 5, T + 9
    crit = LovaszSoftmax("present", per_image=False, ignore_index=L.IGNORE)

    def draw(ignored, absent):
        x = torch.from_numpy((3 * rng.standard_normal((B, N, C))).astype(np.float32)).to(dev)
        t = L._random_target(rng, B * N, C, ignored)
        if absent is not None:
            t[t == absent] = (absent + 1) % C
        return x, torch.from_numpy(t.reshape(B, N)).to(dev)

    x0, t0 = draw(0.1, None)
    xs = x0.clone().requires_grad_(True)
    ts = t0.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            crit(xs.transpose(1, 2), ts).backward()
            xs.grad = None
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_s = crit(xs.transpose(1, 2), ts)
        loss_s.backward()
    for x1, t1 in (draw(0.4, 3), draw(0.0, None)):                        # another count of ignored rows, a class that disappears
        assert int((t1 == L.IGNORE).sum()) != int((t0 == L.IGNORE).sum())
        with torch.no_grad():
            xs.copy_(x1)
        ts.copy_(t1)
        graph.replay()
        torch.cuda.synchronize()
        xe = x1.clone().requires_grad_(True)
        le = crit(xe.transpose(1, 2), t1)
        le.backward()
        assert torch.equal(le.detach().view(torch.int32), loss_s.detach().view(torch.int32))
        assert torch.equal(xe.grad.view(torch.int32), xs.grad.view(torch.int32))
        assert float(le) > 0 and bool(xe.grad.any())


def test_refusals_leave_every_output_untouched(dev):
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    R, C = 8, 3
    x = torch.rand(R, 65, device=dev)
    t = torch.zeros(R, dtype=torch.int64, device=dev)
    ws = torch.full((1 << 16,), SENT, dtype=torch.int32, device=dev)
    for kw in (dict(C=65, ld=65), dict(ld=2), dict(images=3), dict(inner=3), dict(inner=4, images=4), dict(ws_off=4)):
        dpb, dp = _guarded(R * 65, dev)
        pb, prob = _guarded(R * 65, dev)
        lb, loss = _guarded(1, dev)
        c = kw.get("C", C)
        rc = lib.pn2_lovasz_fwd(x.data_ptr(), kw.get("ld", 65), kw.get("inner", 0), t.data_ptr(), R, c, kw.get("images", 1), L.IGNORE, 0,
                                None, 1, ws.data_ptr() + kw.get("ws_off", 0), dp.data_ptr(), prob.data_ptr(), loss.data_ptr(), st)
        torch.cuda.synchronize()
        assert rc == -1, kw                                               # PN2_EINVAL
        assert bool((dpb == SENT).all()) and bool((pb == SENT).all()) and bool((lb == SENT).all()) and bool((ws == SENT).all()), kw
    dxb, dx = _guarded(R * 65, dev)
    assert run_bwd(x, 65, 0, x, R, 65, False, 1.0, dx) == -1 and bool((dxb == SENT).all())
    with pytest.raises(TypeError):
        lovasz_softmax(x.double(), t)
    with pytest.raises(_lib.Pn2Error):
        lovasz_softmax(x, t)                                              # 65 classes
    with pytest.raises(_lib.Pn2Error):
        lovasz_softmax(x[:, :3], t, per_image=True)
    with pytest.raises(_lib.Pn2Error):
        lovasz_softmax(torch.zeros(2, 3, 4, 5, device=dev).permute(0, 1, 3, 2), torch.zeros(2, 5, 4, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        lovasz_softmax(x[:0, :3], t[:0])
    assert ctypes.c_int(lib.pn2_version()).value == 15
