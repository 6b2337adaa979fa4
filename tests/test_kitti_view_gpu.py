"""GPU: the KITTI demo's frame path on the device (pointnet12_amd/kitti_view.py on csrc/view.hip).

Everything here is held EXACTLY.  Predictions and merged classes against ``torch.max`` of the CPU copies; the projection against
what the reference itself returned for the fixture's points (tests/golden/g18_kitti_view.npz) and, off the fixture, against the
restatement that tests/test_kitti_view_cpu.py pins to the reference; the images against the sequential painter of
tests/kitti_view_ref.py, byte for byte.  Shapes are the smallest that reach every path: rows around the 64-lane wave and more
than one 256-thread block, class counts around the float4 quad, images whose pixel count is no multiple of the block."""
import numpy as np
import pytest
import torch

from conftest import golden
import kitti_view_ref as KR

from pointnet12_amd import kitti_view as V
from pointnet12_amd import synthetic as syn

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
I32MIN = KR.INT32_MIN


def G():
    return golden("g18_kitti_view.npz")


def calib(g):
    return V.Calibration(g["R"], g["T"], g["P"])


def same_floats(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# ------------------------------------------------------------------------------------------------------------------ predict
def special_rows(C, rng):
    """Rows that decide the tie and NaN rules: exact ties, all equal, all -inf, a NaN before / after the maximum, two NaNs."""
    rows = [np.full(C, -1.5, np.float32), np.full(C, -INF, np.float32)]
    t = rng.normal(size=C).astype(np.float32)
    t[rng.integers(0, C, 3)] = 7.0                                # the maximum, up to three times
    rows.append(t)
    if C >= 2:
        for nan_at, max_at in ((0, C - 1), (C - 1, 0), (C // 2, C // 2 - 1 if C > 2 else 1)):
            r = rng.normal(size=C).astype(np.float32)
            r[max_at] = 9.0
            r[nan_at] = NAN
            rows.append(r)
        r = rng.normal(size=C).astype(np.float32)
        r[[C // 3, C - 1]] = NAN                                  # two NaNs: the first wins
        rows.append(r)
        r = np.full(C, -INF, np.float32)
        r[C - 1] = -3.0
        rows.append(r)
    return rows


def logp_case(R, C, seed):
    rng = np.random.default_rng(seed)
    lp = np.round(rng.normal(size=(R, C)) * 2).astype(np.float32) / 2          # coarse values: many exact ties
    sp = special_rows(C, rng)
    if R >= len(sp):
        for k, r in enumerate(sp):
            lp[(k * 7) % R] = r
    return lp, sp


def views(lp, dev):
    """The same rows: contiguous; a column slice at an odd offset of a wider buffer (scalar reads); the leading columns of a
    16-byte aligned buffer whose pitch is a multiple of four (float4 reads, the pad holding NaN and +inf)."""
    R, C = lp.shape
    t = torch.from_numpy(lp).to(dev)
    yield "contiguous", t
    wide = torch.full((R, C + 5), NAN, device=dev)
    wide[:, 1::2] = INF
    wide[:, 3:3 + C] = t
    yield "odd slice", wide[:, 3:3 + C]
    ld = (C + 3) // 4 * 4 + 4
    quad = torch.full((R, ld), NAN, device=dev)
    quad[:, C + 1::2] = INF
    quad[:, :C] = t
    yield "quad slice", quad[:, :C]


@pytest.mark.parametrize("C", [1, 2, 19, 64])
def test_predict_equals_torch_max(dev, C):
    for R in (1, 63, 65, 1000):
        lp, sp = logp_case(R, C, 100 * C + R)
        cases = [lp] if R > 1 else [lp] + [r[None] for r in sp]   # one-row inputs: every special row on its own
        for rows in cases:
            ref = torch.from_numpy(rows).max(dim=-1)[1].numpy()
            for name, view in views(rows, dev):
                got = V.predict(view)
                assert got.dtype == torch.int64 and got.shape == (rows.shape[0],)
                assert np.array_equal(got.cpu().numpy(), ref), (R, C, name)
    lp3 = torch.from_numpy(logp_case(130, C, 5)[0]).to(dev).view(2, 65, C)      # [B, N, C] keeps its leading shape
    assert np.array_equal(V.predict(lp3).cpu().numpy(), lp3.cpu().max(dim=-1)[1].numpy())
    out = torch.empty(130, device=dev, dtype=torch.int64)
    assert V.predict(lp3, out=out) is out and np.array_equal(out.cpu().numpy(), lp3.cpu().max(dim=-1)[1].reshape(-1).numpy())
    assert V.predict(torch.empty(0, C, device=dev)).shape == (0,)


def test_merge_classes_and_grouped_predict(dev):
    g = G()
    names, kitti_names = g["class_names"].tolist(), g["kitti_class_names"].tolist()
    tables = [V.merge_groups(names, g["merge_semkitti"].tolist()), V.merge_groups(kitti_names, g["merge_kitti"].tolist()),
              V.merge_groups(names, ["car+truck+other-vehicle", "road", "person+bicyclist"]),          # three members
              V.merge_groups(names, ["terrain"]),                                                     # a single-member table
              V.Groups([0, 19], list(range(18, -1, -1)))]                                             # one group of everything
    assert [len(t) for t in tables[:2]] == [16, 16]
    for R in (1, 65, 1000):
        lp, _ = logp_case(R, 19, 19 + R)
        if R > 1:
            lp[R // 2, :] = NAN
            lp[R // 3, 9:11] = [NAN, 5.0]                          # 'parking+sidewalk': a NaN member beside a large one
        for t in tables:
            members = [t.members(k) for k in range(len(t))]
            ref = KR.merge(lp, members)
            ref_pred = ref.max(dim=-1)[1].numpy()
            for name, view in views(lp, dev):
                m = V.merge_classes(view, t)
                assert m.shape == (R, len(t)) and m.dtype == torch.float32
                assert same_floats(m.cpu().numpy(), ref.numpy()), (R, len(t), name)
                assert np.array_equal(np.isnan(m.cpu().numpy()), np.isnan(ref.numpy()))
                p = V.predict(view, t)
                assert np.array_equal(p.cpu().numpy(), ref_pred), (R, len(t), name)
    with pytest.raises(ValueError):
        V.predict(torch.zeros(4, 13, device=dev), tables[0])      # the table names class 18


# ------------------------------------------------------------------------------------------------------------------ project
def test_projection_is_the_reference_output_bit_for_bit(dev):
    g = G()
    cal, pts, ref = calib(g), g["points"], g["pts_2d"]
    x = torch.from_numpy(pts).to(dev)
    p2, pix = V.project_3d_to_2d(x, cal, return_pixels=True)
    assert p2.dtype == torch.float32 and p2.shape == (2048, 2) and pix.dtype == torch.int32 and pix.shape == (2048, 2)
    assert same_floats(p2.cpu().numpy(), ref)                     # all 2 048 points, the camera-plane one included
    assert np.array_equal(pix.cpu().numpy(), KR.pixels(ref))
    assert (KR.pixels(ref) == I32MIN).any() and (KR.pixels(ref)[:1975] != I32MIN).all()
    assert same_floats(V.torch_project_3d_to_2d(x, cal).cpu().numpy(), ref)
    assert np.array_equal(V.to_pixels(p2).cpu().numpy(), KR.pixels(ref))       # the float -> pixel rule outside the kernel: the same
    only_pix = torch.empty(2048, 2, device=dev, dtype=torch.int32)
    ret = V.project_3d_to_2d(x, cal, out=(None, only_pix))                      # a given pix is filled; the return follows return_pixels
    assert isinstance(ret, torch.Tensor) and same_floats(ret.cpu().numpy(), ref) and np.array_equal(only_pix.cpu().numpy(), KR.pixels(ref))
    both = V.project_3d_to_2d(x, cal, return_pixels=True, out=(ret, None))
    assert both[0] is ret and np.array_equal(both[1].cpu().numpy(), KR.pixels(ref))
    scan = torch.cat([x, torch.full((2048, 1), NAN, device=dev)], 1)            # [N, 4] rows read in place, pitch 4
    p4, pix4 = V.project_3d_to_2d(scan, cal, return_pixels=True)
    assert same_floats(p4.cpu().numpy(), ref) and np.array_equal(pix4.cpu().numpy(), KR.pixels(ref))
    assert same_floats(V.project_3d_to_2d(scan[:, :3], cal).cpu().numpy(), ref)
    one = V.project_3d_to_2d(x[7:8], cal, return_pixels=True)
    assert same_floats(one[0].cpu().numpy(), ref[7:8]) and np.array_equal(one[1].cpu().numpy(), KR.pixels(ref[7:8]))
    none = V.project_3d_to_2d(x[:0], cal, return_pixels=True)
    assert none[0].shape == (0, 2) and none[1].shape == (0, 2)


def test_projection_off_the_fixture_non_finite_and_huge(dev):
    g = G()
    cal = calib(g)
    RT = np.concatenate((g["R"], g["T"]), axis=1)
    rng = np.random.default_rng(3)
    pts = rng.uniform(-80, 80, size=(777, 3)).astype(np.float32)
    pts[:12] = [[INF, 0, 0], [-INF, 1, 1], [NAN, 2, 0], [3, NAN, 0], [3, 0, NAN], [0, 0, 0], [3e38, 3e38, 3e38], [1e-40, 0, 0],
                [5, INF, 0], [5, 0, -INF], [-3e38, 1, 1], [1e30, -1e30, 1e30]]
    with np.errstate(all="ignore"):
        ref = KR.project(pts, RT, g["P"])
    assert (~np.isfinite(ref)).any()
    p2, pix = V.project_3d_to_2d(torch.from_numpy(pts).to(dev), cal, return_pixels=True)
    assert same_floats(p2.cpu().numpy(), ref)
    assert np.array_equal(pix.cpu().numpy(), KR.pixels(ref))
    assert np.array_equal(V.to_pixels(p2).cpu().numpy(), KR.pixels(ref))


# -------------------------------------------------------------------------------------------------------------------- splat
def centres(N, H, W, seed):
    """Disc centres (x, y): corners, edges, 1..4 pixels outside every edge, far away, INT32_MIN, and -- from 4096 points on --
    200 points stacked on 20 pixels so that only the drawing order decides."""
    rng = np.random.default_rng(seed)
    fixed = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2, H - 1), (0, H // 2), (W - 1, H // 2)]
    for d in (1, 2, 3, 4):
        fixed += [(-d, H // 3), (W - 1 + d, H // 3), (W // 3, -d), (W // 3, H - 1 + d), (-d, -d), (W - 1 + d, H - 1 + d)]
    fixed += [(10 ** 6, 5), (5, -10 ** 6), (-10 ** 6, 10 ** 6), (I32MIN, 5), (5, I32MIN), (I32MIN, I32MIN), (2 ** 31 - 1, 2 ** 31 - 1),
              (-2 ** 31 + 1, 3)]
    if N <= 5:
        return np.array(([(0, 0), (W - 1, H - 1), (I32MIN, 3), (W + 1, -2), (1, 1)])[:N], np.int32).reshape(N, 2)
    stack = [(int(rng.integers(0, W)), int(rng.integers(0, H))) for _ in range(20)] * 10
    rest = N - len(fixed) - len(stack)
    rand = np.stack([rng.integers(-6, W + 6, rest), rng.integers(-6, H + 6, rest)], 1)
    pix = np.concatenate([np.array(fixed, np.int64), np.array(stack, np.int64), rand], 0)
    return pix[rng.permutation(N)].astype(np.int32)


@pytest.mark.parametrize("size", [(48, 64), (375, 1242)])
def test_splat_is_the_sequential_painter_byte_for_byte(dev, size):
    H, W = size
    rng = np.random.default_rng(H)
    colors = rng.integers(1, 256, size=(19, 3)).astype(np.uint8)
    background = rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)
    bg_dev = torch.from_numpy(background).to(dev)
    for N in (0, 1, 5, 4096):
        pix = centres(N, H, W, N + W)
        labels = rng.integers(0, 19, N).astype(np.int64)
        if N == 4096:
            labels[:] = np.arange(N) % 19                          # the stacked points carry distinct labels
        pd, ld = torch.from_numpy(pix).to(dev), torch.from_numpy(labels).to(dev)
        for radius, hw in ((2, None), (3, None), (1, [0, 1, 0])):
            table = list(V.DISC_HALF_WIDTHS[radius]) if hw is None else hw
            for bg_np, bg in ((None, None), (background, bg_dev)):
                ref, err = KR.draw(pix, labels, colors, size, table, bg_np)
                assert err == 0
                got = V.draw_2d_points(pd, ld, colors, image=bg, size=size, radius=radius, half_widths=hw)
                assert got.dtype == torch.uint8 and got.shape == (H, W, 3)
                assert np.array_equal(got.cpu().numpy(), ref), (N, radius, bg is not None)
                again = V.draw_2d_points(pd, ld, torch.from_numpy(colors).to(dev), image=bg, size=size, radius=radius, half_widths=hw)
                assert torch.equal(got, again)                     # two runs: byte-identical
        assert np.array_equal(bg_dev.cpu().numpy(), background)         # the background is read, never written


def test_splat_float_centres_preallocated_outputs_and_the_error_flag(dev):
    H, W = 48, 64
    rng = np.random.default_rng(11)
    colors = rng.integers(1, 256, size=(5, 3)).astype(np.uint8)
    pts = rng.uniform(-8, 70, size=(300, 2)).astype(np.float32)
    pts[:6] = [[NAN, 3], [3, INF], [-0.9, -0.9], [63.999, 47.999], [3e9, 1], [-3e9, -INF]]
    labels = rng.integers(0, 5, 300).astype(np.int64)
    ref, _ = KR.draw(KR.pixels(pts), labels, colors, (H, W), V.DISC_HALF_WIDTHS[2])
    out = torch.full((H, W, 3), 77, device=dev, dtype=torch.uint8)
    owner = torch.full((H * W,), -1, device=dev, dtype=torch.int32)     # stale contents: the call clears it itself
    err = torch.zeros(1, device=dev, dtype=torch.int32)
    got = V.draw_2d_points(torch.from_numpy(pts).to(dev), torch.from_numpy(labels).to(dev), colors, size=(H, W), out=out, owner=owner,
                           err=err)
    assert got is out and np.array_equal(out.cpu().numpy(), ref) and int(err.item()) == 0
    # a label equal to C: the pixels it owns keep the background, the flag is set
    bad = labels.copy()
    bad[250:] = 5
    background = rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)
    ref_bad, ref_err = KR.draw(KR.pixels(pts), bad, colors, (H, W), V.DISC_HALF_WIDTHS[2], background)
    assert ref_err == 1 and not np.array_equal(ref_bad, KR.draw(KR.pixels(pts), labels, colors, (H, W), V.DISC_HALF_WIDTHS[2], background)[0])
    got = V.draw_2d_points(torch.from_numpy(pts).to(dev), torch.from_numpy(bad).to(dev), colors, image=torch.from_numpy(background).to(dev),
                           err=err)
    assert np.array_equal(got.cpu().numpy(), ref_bad) and int(err.item()) == 1
    with pytest.raises(IndexError):
        V.draw_2d_points(torch.from_numpy(pts).to(dev), torch.from_numpy(bad).to(dev), colors, size=(H, W))
    with pytest.raises(ValueError):
        V.draw_2d_points(torch.from_numpy(pts).to(dev), torch.from_numpy(labels).to(dev), colors, size=(H, W), radius=4)


# ----------------------------------------------------------------------------------------------------------------- top view
def test_top_view_pixels_and_image(dev):
    rng = np.random.default_rng(21)
    pcd = rng.uniform(-1, 1, size=(1000, 3)).astype(np.float32)
    k = 0
    for offset, col in ((600, 0), (400, 1)):               # -v*800 + offset within one ulp of an integer
        for whole in (0, 1, offset - 1, offset, offset + 1, 799 if col else 599):
            v = np.float32((offset - whole) / 800.0)
            for cand in (np.nextafter(v, np.float32(-2)), v, np.nextafter(v, np.float32(2))):
                pcd[k, col] = cand
                k += 1
    pcd[k:k + 6, :2] = [[1, 1], [-1, -1], [NAN, 0], [0, INF], [3e38, 0], [0.75, -0.5]]
    ref_pix = KR.top_view_pixels(pcd)
    want = [[int(-y * 800 + 400), int(-x * 800 + 600)] for x, y, _ in pcd[:k].tolist()]
    assert np.array_equal(ref_pix[:k], np.array(want))                     # the yardstick itself: Python's int() on tolist() floats
    x = torch.from_numpy(pcd).to(dev)
    pix = V.top_view_pixels(x)
    assert pix.dtype == torch.int32 and np.array_equal(pix.cpu().numpy(), ref_pix)
    assert (ref_pix == I32MIN).any() and ((ref_pix[:, 1] >= 600) & (ref_pix[:, 1] != I32MIN)).any() and (ref_pix[:, 1] < 0).any()
    wide = torch.cat([x, torch.zeros(1000, 1, device=dev)], 1)             # [N, 4] normalised rows, read in place
    assert np.array_equal(V.top_view_pixels(wide).cpu().numpy(), ref_pix)
    colors = rng.integers(1, 256, size=(19, 3)).astype(np.uint8)
    labels = rng.integers(0, 19, 1000).astype(np.int64)
    ref, _ = KR.draw(ref_pix, labels, colors, (600, 800), V.DISC_HALF_WIDTHS[3])
    got = V.draw_2d_top_view(wide, torch.from_numpy(labels).to(dev), colors)
    assert got.shape == (600, 800, 3) and np.array_equal(got.cpu().numpy(), ref)
    un = V.pcd_unnormalize(wide)
    w = wide.cpu().numpy()                                                 # (column 0 holds a NaN: compared as bit patterns)
    ref_un = np.stack([w[:, 0] * np.float32(70), w[:, 1] * np.float32(70), w[:, 2] * np.float32(3), w[:, 3] / np.float32(2) + np.float32(0.5)], 1)
    assert un.shape == wide.shape and same_floats(un.cpu().numpy(), ref_un)


# -------------------------------------------------------------------------------------------------------------------- frame
def test_frame_segmenter(dev):
    from pointnet12_amd.pointnet2 import PointNet2SemSeg
    g = G()
    cal = calib(g)
    names, colors = g["class_names"].tolist(), g["colors"]
    n = syn.kitti_cloud(77, 6000, 6000, 1)[:, :4]
    scan = np.stack([n[:, 0] * 70, n[:, 1] * 70, n[:, 2] * 3, n[:, 3] / 2 + 0.5], 1).astype(np.float32)
    torch.manual_seed(0)
    model = PointNet2SemSeg(19, feature_dims=1).to(dev).eval()
    seg = V.FrameSegmenter(model, cal, colors, npoints=2048, image_size=(375, 1242))
    choice = np.random.default_rng(5).integers(0, len(scan), 2048)
    background = np.random.default_rng(6).integers(0, 256, size=(375, 1242, 3)).astype(np.uint8)
    out = seg.frame(scan, background=torch.from_numpy(background).to(dev), choice=choice)
    lp = out["log_probs"]
    assert lp.shape == (2048, 19) and not model.training
    pred = out["pred"].cpu().numpy()
    assert np.array_equal(pred, lp.cpu().max(dim=-1)[1].numpy())
    picked = scan[choice]
    assert np.array_equal(out["pts_3d"].cpu().numpy().view(np.uint32), picked[:, :3].view(np.uint32))
    normed = np.clip(np.stack([picked[:, 0] / np.float32(70), picked[:, 1] / np.float32(70), picked[:, 2] / np.float32(3),
                               (picked[:, 3] - np.float32(0.5)) * np.float32(2)], 1), -1, 1)
    assert same_floats(out["points"].cpu().numpy(), normed)
    RT = np.concatenate((g["R"], g["T"]), axis=1)
    ref2d = KR.project(picked[:, :3], RT, g["P"])
    assert same_floats(out["pts_2d"].cpu().numpy(), ref2d)
    # teacher-forced: the restatement draws with the pipeline's own predictions, so network noise is out of the comparison
    ref_img, _ = KR.draw(KR.pixels(ref2d), pred, colors, (375, 1242), V.DISC_HALF_WIDTHS[2], background)
    ref_top, _ = KR.draw(KR.top_view_pixels(normed), pred, colors, (600, 800), V.DISC_HALF_WIDTHS[3])
    assert np.array_equal(out["image"].cpu().numpy(), ref_img) and not np.array_equal(ref_img, background)
    assert np.array_equal(out["top_view"].cpu().numpy(), ref_top) and ref_top.any()
    assert int(seg.error_flag.item()) == 0
    eager_img, eager_top, eager_pred = out["image"].clone(), out["top_view"].clone(), out["pred"].clone()

    # the post-network stages captured into a graph and replayed twice give the eager bytes
    lp_static, raw_static, pts_static = lp.clone(), seg.raw_rows.clone(), out["points"].clone()
    bg_static = torch.from_numpy(background).to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        seg.render(lp_static, raw_static, pts_static, bg_static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        seg.render(lp_static, raw_static, pts_static, bg_static)
    for _ in range(2):
        seg.image.zero_()
        seg.top_view.zero_()
        seg.pred.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(seg.image, eager_img) and torch.equal(seg.top_view, eager_top) and torch.equal(seg.pred, eager_pred)

    # with a merge list the prediction is a merged class
    groups = V.merge_groups(names, g["merge_semkitti"].tolist(), colors)
    merged = V.FrameSegmenter(model, cal, groups.colors, npoints=2048, groups=groups)
    out2 = merged.frame(torch.from_numpy(scan), choice=torch.from_numpy(choice))
    p2 = out2["pred"].cpu().numpy()
    assert p2.min() >= 0 and p2.max() < 16
    ref_merged = KR.merge(out2["log_probs"].cpu().numpy(), [groups.members(k) for k in range(16)])
    assert np.array_equal(p2, ref_merged.max(dim=-1)[1].numpy())
    ref_img2, _ = KR.draw(KR.pixels(ref2d), p2, groups.colors, (375, 1242), V.DISC_HALF_WIDTHS[2])
    assert np.array_equal(out2["image"].cpu().numpy(), ref_img2)
    # a seeded numpy draw is the reference's draw (pcdvis.py:121)
    np.random.seed(4)
    drawn = merged.choice(len(scan)).cpu().numpy()
    np.random.seed(4)
    assert np.array_equal(drawn, np.random.choice(len(scan), 2048, replace=True))
    # the error flag is per frame: a choice outside the scan sets it, the next good frame starts from zero
    bad_choice = choice.copy()
    bad_choice[17] = len(scan)
    merged.frame(scan, choice=bad_choice)
    assert int(merged.error_flag.item()) == 1
    merged.frame(scan, choice=choice)
    assert int(merged.error_flag.item()) == 0
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    c = merged.choice(len(scan), gen)
    assert c.shape == (2048,) and int(c.min()) >= 0 and int(c.max()) < len(scan)
