"""GPU: the colour-generation task above the kernels -- PointNetColorGen against the fp64 restatement, prepare_color_batch against
the numpy statement of ColorGeneratorLoader.__getitem__, paint_points, FrameSegmenter(image=) and per-point-colour drawing."""
import os

import numpy as np
import pytest
import torch

import image_sample_ref as R
import pointnet_v1_ref as V
from conftest import GOLDEN, golden
from oracle import train_ref as T
from test_pointnet_v1_cpu import bias_before_bn

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------------------------------------------------- model
def colorgen_forward(P, x, train, feature_transform, pick):
    """PointNetColorGen on the restatement's pieces: seg_forward (pointnet_v1_ref.py) without its log-softmax.
    x [B, C, N] -> (out [B, N, k], trans_feat)."""
    g, pf, _, trans_feat = V.encoder(P, "feat.", x.transpose(1, 2), train, feature_transform, "factorised", pick)
    w1 = P["conv1.weight"].reshape(P["conv1.weight"].shape[0], -1)
    cg = g.shape[1]
    y1 = pf @ w1[:, cg:].transpose(0, 1) + (g @ w1[:, :cg].transpose(0, 1))[:, None, :] + P["conv1.bias"]
    h = torch.relu(V._norm(P, "bn1", y1, train))
    h = V._unit(P, "conv2", "bn2", h, train)
    h = V._unit(P, "conv3", "bn3", h, train)
    return V._linear(P, "conv4", h), trans_feat


def zero_in_exact_arithmetic(key):
    """Training mode: biases whose gradient is zero up to rounding, compared on their weight's scale (the rule of
    tests/test_pointnet_v1_cpu.py for a conv / fc bias in front of a BatchNorm).  The same holds for the bias of each ``bn3`` in
    front of a max over the points: it adds one constant per channel to every cloud's maximum, and the next layer ends in a
    training-mode BatchNorm over the clouds (fc1 + bn4 in both STNs) or over all rows (the head's conv1 + bn1), which removes it.
    THIS GOES BEYOND THE RULE AS THE PROJECT HAS IT: tests/test_pointnet_v1_gpu.py holds these three biases to their own scale.  It
    applies in training mode only."""
    return bias_before_bn(key) or key in ("feat.stn.bn3.bias", "feat.fstn.bn3.bias", "feat.bn3.bias")


PAIR_BAND = (0.03, 0.05)


def separate_pairs(sd, x, ft):
    """The test's WEIGHTS, chosen so that a batch of two clouds is a problem fp32 can be held to.  With B = 2 the training-mode
    BatchNorms behind fc1 / fc2 of both STNs normalise PAIRS: a channel with pre-BN values a_0, a_1 gives xhat = +-d / sqrt(d^2 + eps),
    d = (a_0 - a_1) / 2.  Forward, its derivative eps / (d^2 + eps)^1.5 reaches 1 / sqrt(eps) = 316 at d = 0 and falls below 1 only
    for |d| > 0.0215; backward, the gradient is g (1 - xhat^2) = g eps / (d^2 + eps), formed as a difference of terms of size g, so
    its relative error is fp32's 6e-8 divided by 1 - xhat^2.  With stock initial weights d is about N(0, 0.4): some 4 % of the 1536
    pair channels amplify whatever rounding reaches them (stock torch fp32 itself then lands up to a third of a tensor's largest
    entry away from fp64) and in most of the others 1 - xhat^2 is 1e-4 and less; a comparison then measures which evaluation was
    luckier in one channel, or which BatchNorm backward formula cancels better.  So every pair channel is moved into
    PAIR_BAND, 0.03 <= |d| <= 0.05: amplification at most 0.36 forward, 1 - xhat^2 at least 4e-3 backward (relative error 2e-5 at
    most, below the 3e-5 of the rule).  The row w_c of the layer's weight takes the smallest change along dv = (v_0 - v_1) / 2, its
    input's pair difference, that puts d_c = w_c . dv at +-clamp(|d_c|, 0.0375, 0.045) (the margins cover the float32 rounding of
    the new row; the bias cancels in d).  The layer's BIAS then centres each pair, a_0 = +d and a_1 = -d: the variance of two
    values is then d^2 itself, however it is formed.  (These four BatchNorms are torch's own ``nn.BatchNorm1d`` on ``[2, C]`` inside
    the networks, no kernel of this library; with uncentred pairs the networks' gradients through them sat 5 to 70 times further
    from fp64 than the restatement's explicit formula in stock fp32, at 1e-4 to 5e-4 of scale.  A variance formed as E[a^2] - E[a]^2
    would do that -- a supposition, torch's kernel was not read.  A two-cloud training batch is no use case of the reference's
    drivers, which train on 8 to 32 clouds.)  Everything is computed from the fp64 restatement on the host, layer after layer, before
    the library sees anything.  Returns the new state dict."""
    sd = dict(sd)
    with torch.no_grad():
        P = V.Params(sd, torch.float64, "cpu")

        def head(pre, rows):
            h = rows
            for i in (1, 2, 3):
                h = V._unit(P, pre + "conv%d" % i, pre + "bn%d" % i, h, True)
            v = h.amax(dim=1)
            for fc, bn in (("fc1", "bn4"), ("fc2", "bn5")):
                key = pre + fc + ".weight"
                w, dv = P[key], (v[0] - v[1]) / 2
                d = w @ dv
                target = d.abs().clamp(1.25 * PAIR_BAND[0], 0.9 * PAIR_BAND[1]) * torch.where(d < 0, -1.0, 1.0)
                w = (w + ((target - d) / (dv @ dv))[:, None] * dv[None, :]).float()
                sd[key], P.p[key] = w, w.double()
                bias = (-(P[key] @ ((v[0] + v[1]) / 2))).float()         # the pair centred: a_0 = +d, a_1 = -d
                sd[pre + fc + ".bias"], P.p[pre + fc + ".bias"] = bias, bias.double()
                assert PAIR_BAND[0] <= float((P[key] @ dv).abs().min()) and float((P[key] @ dv).abs().max()) <= PAIR_BAND[1]
                v = V._unit(P, pre + fc, pre + bn, v, True)

        rows = x.double().transpose(1, 2)
        head("feat.stn.", rows)
        if ft:
            trans = V.stn(P, "feat.stn.", rows, True, rows.shape[-1])
            head("feat.fstn.", V._unit(P, "feat.conv1", "feat.bn1", V._apply(rows, trans, "factorised"), True))
    return sd


def restated(sd, x, gw, train, ft, dtype, dev, pick):
    P = V.Params(sd, dtype, dev)
    xx = x.to(dtype).detach().requires_grad_(True)
    out, tf = colorgen_forward(P, xx, train, ft, pick)
    loss = (out * gw.to(dtype)).sum()
    if ft:
        loss = loss + 0.001 * V.regulariser(tf)
    loss.backward()
    res = {"out": out.detach(), "grad/x": xx.grad}
    if ft:
        res["trans_feat"] = tf.detach()
    res.update({"grad/" + k: v for k, v in P.grads().items()})
    if train:
        res.update({"after/" + k: v for k, v in P.state.items() if k.endswith(("running_mean", "running_var"))})
    return res


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("ft", [False, True], ids=["plain", "feature_transform"])
def test_colorgen_against_fp64(dev, ft, train):
    """B = 2, N = 70, input_dims 4, k = 3: the output and every gradient within 3e-5 of the tensor's largest entry or within 4x of
    what stock torch fp32 achieves on the same restatement (the rule of tests/test_pointnet_v1_glue_gpu.py).  Every figure is
    printed before it is held to the bound.

    The STN heads' fc1 / fc2 weights and biases come from ``separate_pairs``: with stock initial weights a two-cloud training step is
    so badly conditioned (stock torch fp32 up to a third of a tensor's largest entry away from fp64) that the comparison would
    measure rounding luck in single channels; with every pair channel centred and inside PAIR_BAND stock fp32 lands within 1e-4 of
    scale and the rule means something.  The shapes, the modes and the bound are as the issue sets them."""
    from pointnet12_amd import pointnet as M
    B, N, k = 2, 70, 3
    torch.manual_seed(11 + ft)
    net = M.PointNetColorGen(k, 4, ft)
    gen = torch.Generator(device="cpu").manual_seed(5)
    sd = {}
    for key, v in net.state_dict().items():                          # running statistics that an eval pass can get wrong
        if key.endswith("running_mean"):
            v = 0.1 * torch.randn(v.shape, generator=gen)
        elif key.endswith("running_var"):
            v = 0.5 + torch.rand(v.shape, generator=gen)
        sd[key] = v.detach().clone()
    x = torch.randn(B, 4, N, generator=gen)
    gw = torch.randn(B, N, k, generator=gen).to(dev)
    sd = separate_pairs(sd, x, ft)
    x = x.to(dev)
    net.load_state_dict(sd)
    net.to(dev).train(train)
    # the library's arg-max rows of the max-pools over the points (STN, feature STN, encoder): where two points tie to within
    # rounding the gradient follows whichever row was picked, and any of the tied rows is a right answer -- both restatements are
    # evaluated at the library's choice, as tests/test_pointnet_v1_gpu.py does
    picks = {}
    orig_mlp, orig_max = M.shared_mlp, M.conv_bn_max

    def spy_mlp(rows, c_in, convs, bns, pool, training, dest=None):
        out = orig_mlp(rows, c_in, convs, bns, pool, training, dest)
        if pool:
            site = "feat.fstn." if "feat.stn." in picks else "feat.stn."
            picks[site] = out.grad_fn.saved_tensors[2][:, :out.shape[1]].long().view(B, -1)
        return out

    def spy_max(x, conv, bn, N, training):
        out = orig_max(x, conv, bn, N, training)
        picks["feat."] = out.grad_fn.saved_tensors[3][:, :out.shape[1]].long().view(B, -1)
        return out
    M.shared_mlp, M.conv_bn_max = spy_mlp, spy_max
    try:
        xx = x.clone().requires_grad_(True)
        out, tf = net(xx)
    finally:
        M.shared_mlp, M.conv_bn_max = orig_mlp, orig_max
    assert sorted(picks) == (["feat.", "feat.fstn.", "feat.stn."] if ft else ["feat.", "feat.stn."])
    assert out.shape == (B, N, k) and (tf is None) == (not ft)
    # the k columns are a slice of the padded rows the last GEMM wrote: pitch round4(k), no copy
    assert out.stride() == (N * 4, 4, 1)
    loss = (out * gw).sum()
    if ft:
        loss = loss + 0.001 * M.feature_transform_reguliarzer(tf)
    loss.backward()
    got = {"out": out.detach(), "grad/x": xx.grad}
    if ft:
        got["trans_feat"] = tf.detach()
    got.update({"grad/" + key: p.grad for key, p in net.named_parameters()})
    if train:
        got.update({"after/" + key: b for key, b in net.named_buffers() if key.endswith(("running_mean", "running_var"))})
    ref = restated(sd, x, gw, train, ft, torch.float64, dev, picks)
    f32 = restated(sd, x, gw, train, ft, torch.float32, dev, picks)
    assert sorted(got) == sorted(ref)
    bad = []
    for key, r in ref.items():
        assert got[key] is not None and got[key].shape == r.shape, key
        scale = float(r.abs().max())
        if train and key.startswith("grad/") and zero_in_exact_arithmetic(key[len("grad/"):]):
            scale = float(ref[key[:-len("bias")] + "weight"].abs().max())       # exactly 0: held to the weight's scale
        err, err32 = float((got[key].double() - r).abs().max()), float((f32[key].double() - r).abs().max())
        print("%-34s err %.3e  stock fp32 %.3e  scale %.3e" % (key, err, err32, scale))
        if not err <= max(3e-5 * scale, 4.0 * err32):
            bad.append((key, err, err32, scale))
    assert not bad, bad
    if not train:                                                     # the inference path (no autograd: the fused eval kernels)
        with torch.no_grad():
            out2, _ = net(x)
        err = float((out2.double() - ref["out"]).abs().max())
        assert err <= max(3e-5 * float(ref["out"].abs().max()), 4.0 * float((f32["out"].double() - ref["out"]).abs().max()))


# ----------------------------------------------------------------------------------------------------------------------- batch
NPOINTS = 16
LENGTHS = [NPOINTS, NPOINTS + 1, 2 * NPOINTS, NPOINTS - 1, NPOINTS // 2, 3]


def color_store(dev):
    from pointnet12_amd import loader
    rng = np.random.RandomState(2)
    store = loader.ColorStore(LENGTHS, dev)
    rows = sum(LENGTHS)
    raw = (rng.uniform(-1, 1, (rows, 4)) * [80, 80, 4, 1]).astype(np.float32)         # beyond the clip of pcd_normalize too
    color = rng.uniform(0, 1, (rows, 3)).astype(np.float32)
    store.raw.copy_(torch.from_numpy(raw))
    store.color.copy_(torch.from_numpy(color))
    assert store.color.data_ptr() == store.raw.data_ptr() + rows * 16                # back to back in one allocation
    return store, raw, color


def getitem(raw, color, npoints, train):
    """ColorGeneratorLoader.__getitem__ (ColorGenerator_Loader.py:82-101) on one cached item, in numpy."""
    pcd = T.normalize(raw)
    if train:
        pcd = T.jitter_noise(pcd.shape[0], 4) + pcd
    if 2 * pcd.shape[0] >= npoints:
        return R.window_item(pcd, color, npoints)
    rows = R.window_rows(pcd.shape[0], npoints, 0)                   # (the reference's item is short here: the wrap continues it)
    return pcd[rows], color[rows]


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("static", [False, True], ids=["fresh", "out"])
def test_prepare_color_batch_is_getitem_bit_for_bit(dev, train, static):
    from pointnet12_amd import loader
    store, raw, color = color_store(dev)
    ids = [3, 0, 5, 2, 1, 4, 2]
    begins = np.cumsum(LENGTHS) - LENGTHS
    for seed in (0, 1):
        np.random.seed(seed)
        want = [getitem(raw[begins[i]:begins[i] + LENGTHS[i]], color[begins[i]:begins[i] + LENGTHS[i]], NPOINTS, train) for i in ids]
        np.random.seed(seed)
        out = None
        if static:
            out = (torch.full((len(ids), NPOINTS, 4), 7.0, device=dev), torch.full((len(ids), NPOINTS, 3), 7.0, device=dev))
        pts, tgt = loader.prepare_color_batch(store, ids, NPOINTS, train, "numpy", out=out)
        if static:
            assert pts is out[0] and tgt is out[1]
        assert pts.shape == (len(ids), NPOINTS, 4) and tgt.shape == (len(ids), NPOINTS, 3)
        assert pts.cpu().numpy().tobytes() == np.stack([w[0] for w in want]).astype(np.float32).tobytes()
        assert tgt.cpu().numpy().tobytes() == np.stack([w[1] for w in want]).astype(np.float32).tobytes()


def test_prepare_color_batch_device_generator(dev):
    """The device draw: every item is a window of its cloud (normalised, no jitter), its start inside the reference's range."""
    from pointnet12_amd import loader
    store, raw, color = color_store(dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    ids = [2] * 40 + [1, 0, 3, 4, 5]
    pts, tgt = loader.prepare_color_batch(store, ids, NPOINTS, False, gen)
    begins = np.cumsum(LENGTHS) - LENGTHS
    starts = set()
    for b, i in enumerate(ids):
        M = LENGTHS[i]
        c = color[begins[i]:begins[i] + M]
        first = int(np.where((c == tgt[b, 0].cpu().numpy()).all(1))[0][0])
        assert first == 0 or M > NPOINTS
        assert 0 <= first <= max(M - NPOINTS - 1, 0)
        rows = R.window_rows(M, NPOINTS, first)
        assert tgt[b].cpu().numpy().tobytes() == c[rows].tobytes()
        assert pts[b].cpu().numpy().tobytes() == T.normalize(raw[begins[i]:begins[i] + M])[rows].tobytes()
        if i == 2:
            starts.add(first)
    assert len(starts) > 5                                            # 40 draws out of 16 starts


# ----------------------------------------------------------------------------------------------------------------------- paint
def calibration():
    from pointnet12_amd import kitti_view as KV
    if os.path.exists(os.path.join(GOLDEN, "g18_kitti_view.npz")):
        g = golden("g18_kitti_view.npz")
        return KV.Calibration(g["R"], g["T"], g["P"]), g["points"][:, :3].astype(np.float32)
    R_ = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
    P_ = np.array([[720.0, 0.0, 610.0], [0.0, 720.0, 175.0], [0.0, 0.0, 1.0]])
    rng = np.random.RandomState(0)
    pts = np.stack([rng.uniform(2, 60, 3000), rng.uniform(-30, 30, 3000), rng.uniform(-3, 2, 3000)], 1).astype(np.float32)
    return KV.Calibration(R_, np.array([[0.0], [-0.08], [-0.27]]), P_), pts


def test_paint_points_is_project_then_sample(dev):
    from pointnet12_amd import kitti_view as KV
    cal, xyz = calibration()
    rng = np.random.RandomState(1)
    M = len(xyz)
    scan = np.concatenate([xyz, rng.uniform(0, 1, (M, 1)).astype(np.float32)], 1)
    scan[:5, :3] = [[0, 0, 0], [-10, 0, 0], [-10, 1, 0.5], [np.nan, 1, 1], [1e30, 1e30, 1]]      # on / behind the camera, not finite
    image_np = rng.randint(0, 256, (375, 1242, 3)).astype(np.uint8)
    pts, image = torch.from_numpy(scan).to(dev), torch.from_numpy(image_np).to(dev)
    for mode, norm, order in (("hsv", True, "rgb"), ("rgb", False, "bgr")):
        _, pix = KV.project_3d_to_2d(pts, cal, return_pixels=True)
        colors, valid = KV.sample_image(pix, image, mode, norm, order)
        painted, pvalid = KV.paint_points(pts, cal, image, mode, norm, order, return_valid=True)
        assert painted.shape == (M, 7)
        assert torch.equal(painted[:, :4].view(torch.int32), pts.view(torch.int32))
        assert torch.equal(painted[:, 4:].contiguous().view(torch.int32), colors.view(torch.int32)) and torch.equal(pvalid, valid)
        want, want_valid = R.sample_image(pix.cpu().numpy(), image_np, mode, norm, order)
        assert colors.cpu().numpy().tobytes() == want.tobytes() and (valid.cpu().numpy() == want_valid).all()
        assert 0 < int(valid.sum()) < M
        # into wide rows that already hold the points, with every buffer given: the columns are painted in place
        rows = torch.full((M, 7), -5.0, device=dev)
        rows[:, :4] = pts
        pix2, valid2 = torch.empty(M, 2, device=dev, dtype=torch.int32), torch.empty(M, device=dev, dtype=torch.uint8)
        again = KV.paint_points(rows[:, :4], cal, image, mode, norm, order, out=rows, pix=pix2, valid=valid2)
        assert again is rows and torch.equal(rows.view(torch.int32), painted.view(torch.int32)) and torch.equal(pix2, pix)
        # float pixel coordinates go through to_pixels
        c2, v2 = KV.sample_image(KV.project_3d_to_2d(pts, cal), image, mode, norm, order)
        assert torch.equal(c2.view(torch.int32), colors.view(torch.int32)) and torch.equal(v2, valid)
    # the way back: the stored target of an in-image point, seen again, is its pixel to within the 8-bit HSV quantisation
    hsv, valid = KV.sample_image(pix, image, "hsv", True, "rgb")
    back = KV.hsv_to_rgb(hsv)
    assert back.shape == (M, 3) and back.dtype == torch.uint8
    assert back.cpu().numpy().tobytes() == R.hsv_to_rgb(hsv.cpu().numpy()).tobytes()
    wide = torch.zeros(M, 7, device=dev)
    wide[:, 4:] = hsv
    assert torch.equal(KV.hsv_to_rgb(wide[:, 4:], "bgr"), back.flip(-1))


def test_color_store_from_scans(dev):
    from pointnet12_amd import kitti_view as KV, loader
    cal, xyz = calibration()
    rng = np.random.RandomState(4)
    scans = [np.concatenate([xyz[a:b], rng.uniform(0, 1, (b - a, 1)).astype(np.float32)], 1) for a, b in ((0, 700), (700, 701), (701, 1500))]
    images = [rng.randint(0, 256, (375, 1242, 3)).astype(np.uint8) for _ in scans]
    for chunk_rows in (1 << 22, 1):                                   # one batched call, and one call per scan
        store = loader.ColorStore.from_scans(scans, images, cal, chunk_rows=chunk_rows, device=dev)
        assert store.row_count.tolist() == [700, 1, 799] and len(store) == 3
        at = 0
        for s, img in zip(scans, images):
            _, pix = KV.project_3d_to_2d(torch.from_numpy(s).to(dev), cal, return_pixels=True)
            want, want_valid = R.sample_image(pix.cpu().numpy(), img, "hsv", True, "rgb")
            n = len(s)
            assert store.raw[at:at + n].cpu().numpy().tobytes() == s.tobytes()
            assert store.color[at:at + n].cpu().numpy().tobytes() == want.tobytes()
            assert (store.valid[at:at + n].cpu().numpy() == want_valid).all()
            at += n


# ----------------------------------------------------------------------------------------------------------------------- frame
def test_frame_segmenter_with_an_image(dev):
    from pointnet12_amd import kitti_view as KV, synthetic as syn
    from pointnet12_amd.pointnet import PointNetSeg
    cal, _ = calibration()
    scan = syn.kitti_scan(77, 3000)
    torch.manual_seed(0)
    model = PointNetSeg(19, 4).to(dev).eval()
    colors = np.random.RandomState(0).randint(0, 256, (19, 3)).astype(np.uint8)
    image_np = np.random.RandomState(1).randint(0, 256, (375, 1242, 3)).astype(np.uint8)
    image = torch.from_numpy(image_np).to(dev)
    choice = np.random.RandomState(2).randint(0, len(scan), 1024)
    seg = KV.FrameSegmenter(model, cal, colors, npoints=1024, color_mode="hsv")
    plain = {k: v.clone() for k, v in seg.frame(scan, choice=choice).items()}
    assert "point_colors" not in plain and "point_valid" not in plain and seg.point_colors is None
    out = seg.frame(scan, choice=choice, image=image)
    assert sorted(out) == sorted(list(plain) + ["point_colors", "point_valid"])
    for k, v in plain.items():
        assert v.dtype == out[k].dtype and v.shape == out[k].shape, k
        assert bytes(v.contiguous().view(torch.uint8).cpu().numpy().tobytes()) == out[k].contiguous().view(torch.uint8).cpu().numpy().tobytes(), k
    want, want_valid = R.sample_image(out["pix"].cpu().numpy(), image_np, "hsv", True, "rgb")
    assert out["point_colors"].cpu().numpy().tobytes() == want.tobytes()
    assert out["point_valid"].dtype == torch.bool and (out["point_valid"].cpu().numpy() == want_valid).all()
    assert int(seg.error_flag.item()) == 0
    again = seg.frame(scan, choice=choice)                            # and image=None afterwards is the plain call again
    assert sorted(again) == sorted(plain)


# ------------------------------------------------------------------------------------------------------------------------ draw
def test_draw_with_a_colour_per_point(dev):
    from pointnet12_amd import kitti_view as KV
    rng = np.random.RandomState(9)
    N = 300
    pix = torch.from_numpy(np.stack([rng.randint(-5, 70, N), rng.randint(-5, 45, N)], 1).astype(np.int32)).to(dev)
    colors = torch.from_numpy(rng.randint(0, 256, (N, 3)).astype(np.uint8)).to(dev)
    background = torch.from_numpy(rng.randint(0, 256, (40, 64, 3)).astype(np.uint8)).to(dev)
    for bg in (None, background):
        a = KV.draw_2d_points(pix, None, colors, bg, (40, 64))
        b = KV.draw_2d_points(pix, torch.arange(N, device=dev), colors, bg, (40, 64))
        assert torch.equal(a, b) and bool((a != (0 if bg is None else bg)).any())
    with pytest.raises(ValueError):
        KV.draw_2d_points(pix, None, colors[:19], None, (40, 64))
    # a prediction drawn: hsv_to_rgb's pixels as the per-point colours
    hsv = torch.from_numpy(rng.uniform(0, 1, (N, 3)).astype(np.float32)).to(dev)
    img = KV.draw_2d_points(pix, None, KV.hsv_to_rgb(hsv), None, (40, 64))
    assert img.shape == (40, 64, 3) and bool(img.any())
