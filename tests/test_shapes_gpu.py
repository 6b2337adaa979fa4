"""GPU: pn2_prepare_shapes and pointnet12_amd/shapes.py -- bit for bit against what the REFERENCE's ShapeNet-part / ModelNet / S3DIS
items are (tests/golden/g17_shapes.npz, recorded by tools/make_golden_shapes.py) and against tests/shapes_ref.py."""
import os

import numpy as np
import pytest
import torch

import shapes_ref as SR
from conftest import GOLDEN, golden
from pointnet12_amd import _lib, s3dis, shapes

pytestmark = pytest.mark.gpu

TREE = os.path.join(GOLDEN, "g17_shapenet")
MNET = os.path.join(GOLDEN, "g17_modelnet")
_p = _lib.ptr


def bits(a):
    if torch.is_tensor(a):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def eq(a, b):
    return bool((bits(a) == bits(b)).all())


# ------------------------------------------------------------------------------------------------ golden
def test_shapenet_items_golden_bit_exact(dev):
    g = golden("g17_shapes.npz")
    sets = {(s, n): shapes.ShapeNetPart(TREE, s, normalize=n, device=dev) for s in ("trainval", "test") for n in (True, False)}
    seen = set()
    for tag in g["shapenet/cases"]:
        ds = sets[str(g[tag + "/split"]), bool(g[tag + "/normalize"])]
        ds.npoints = int(g[tag + "/npoints"])
        np.random.seed(int(g[tag + "/seed"]))
        pts, cls, seg, nrm = ds.batch([int(g[tag + "/index"])], augment=bool(g[tag + "/augment"]))
        assert pts.shape == (1, ds.npoints, 3) and nrm.shape == (1, ds.npoints, 3) and seg.dtype == torch.int64 and cls.dtype == torch.int64
        assert eq(pts[0], g[tag + "/points"]), tag
        assert eq(nrm[0], g[tag + "/normals"]), tag
        assert (seg[0].cpu().numpy() == g[tag + "/seg"]).all(), tag
        assert cls.cpu().numpy().tolist() == g[tag + "/cls"].tolist(), tag
        seen.add((int(g[tag + "/M"]), ds.npoints))
    assert {m for m, _ in seen} >= {2, 63, 64, 65, 300} and {n for _, n in seen} >= {1, 64, 255, 257, 2048}


def test_modelnet_items_golden_bit_exact(dev):
    g = golden("g17_shapes.npz")
    ds = shapes.ModelNet40(MNET, train=False, device=dev)
    for i in (0, 4):
        pts, lab = ds.batch([i], augment=False)
        assert pts.shape == (1, 2048, 3) and eq(pts[0], ds.data[i]) and int(lab[0]) == int(ds.labels[i, 0])
        np.random.seed(int(g["modelnet/item%d/seed" % i]))
        pts, lab = ds.batch([i], augment=True)
        assert eq(pts[0], g["modelnet/item%d/augmented" % i]) and int(lab[0]) == int(g["modelnet/label"][i, 0])


def test_s3dis_block_golden_bit_exact(dev):
    g = golden("g17_shapes.npz")
    d0, l0 = s3dis.load_h5(os.path.join(GOLDEN, "g11_s3dis", "ply_data_all_0.h5"))
    st = shapes.S3DISStore(d0, l0, device=dev)
    k = int(g["s3dis/block"])
    np.random.seed(int(g["s3dis/seed"]))
    pts, lab = st.batch([k], augment=True)
    assert pts.shape == (1, 4096, 9) and eq(pts[0], g["s3dis/jittered"]) and (lab[0].cpu().numpy() == l0[k]).all()
    np.random.seed(int(g["s3dis/seed"]))                        # ... which is s3dis.S3DISDataLoader's item as well
    assert eq(pts[0], s3dis.S3DISDataLoader(d0, l0, True)[k][0])
    pts, lab = st.batch([2, 0], augment=False)
    assert eq(pts, d0[[2, 0]]) and (lab.cpu().numpy() == l0[[2, 0]]).all()


# ------------------------------------------------------------------------------------------------ order of the draws
@pytest.mark.parametrize("augment", [True, False])
def test_ragged_batch_matches_sequential_getitem(dev, augment):
    """A ragged batch (a shape twice, B no power of two) draws cloud by cloud in the order a num_workers=0 DataLoader calls
    __getitem__: angle, noise, choice per item."""
    ds = shapes.ShapeNetPart(TREE, "trainval", npoints=257, device=dev)
    order = [3, 0, 2, 0]
    assert len({len(ds.arrays[i]) for i in order}) == 3
    np.random.seed(77)
    ref = [SR.shapenet_item(ds.arrays[i], ds.cls_ids[i], 257, True, augment) for i in order]
    np.random.seed(77)
    pts, cls, seg, nrm = ds.batch(order, augment=augment)
    for b in range(len(order)):
        assert eq(pts[b], ref[b][0]) and eq(nrm[b], ref[b][3]), b
        assert (seg[b].cpu().numpy() == ref[b][2]).all() and int(cls[b]) == int(ref[b][1][0]), b


# ------------------------------------------------------------------------------------------------ the entry point itself
def synthetic_store(dev, B=8, C=6, lo=2600, hi=2800, seed=3):
    """Shapes of lo .. hi points; column 3 holds the row number, column 4 the shape number (both exact in fp32)."""
    rng = np.random.default_rng(seed)
    clouds, segs = [], []
    for b in range(B):
        m = int(rng.integers(lo, hi + 1))
        c = rng.uniform(-1, 1, (m, C)).astype(np.float32)
        c[:, 3], c[:, 4] = np.arange(m), b
        clouds.append(c)
        segs.append(((np.arange(m) * 7 + b) % 50).astype(np.int32))
    return shapes.ShapeStore(clouds, segs, np.arange(B) % 16, dev), clouds, segs


def launch(store, d, N, out, labels=None, bad=None):
    return _lib.load().pn2_prepare_shapes(_p(store.raw), store.C, _p(d.begin), _p(d.count), _p(store.label), _p(d.rot), _p(d.noise),
                                          d.noise_cols, _p(d.noise_begin), _p(d.choice), d.ids.numel(), N, _p(out), _p(labels),
                                          _p(bad), _lib.stream())


def test_identity_choice_equals_explicit_arange(dev):
    store, clouds, _ = synthetic_store(dev, B=3, C=9, lo=300, hi=333)
    np.random.seed(5)
    d = shapes.draw(store, [2, 0, 1], None, rotate=True, jitter=True, noise_cols=4)
    N = 300
    assert d.choice is None
    a = torch.empty(3, N, 9, device=dev)
    b = torch.empty(3, N, 9, device=dev)
    la = torch.empty(3, N, dtype=torch.int64, device=dev)
    lb = torch.empty(3, N, dtype=torch.int64, device=dev)
    assert launch(store, d, N, a, la) == 0
    ar = torch.arange(N, device=dev).repeat(3, 1).contiguous()
    assert launch(store, d._replace(choice=ar), N, b, lb) == 0
    assert eq(a, b) and torch.equal(la, lb)
    raw = np.stack([clouds[i][:N] for i in (2, 0, 1)])
    assert eq(a[..., 4:], raw[..., 4:])                          # columns >= noise_cols: bit copies
    noise, begin, cs = d.noise.cpu().numpy(), d.noise_begin.cpu().numpy(), d.rot.cpu().numpy()
    for k in range(3):                                           # columns < noise_cols: rotated (0..2) and jittered (0..3)
        nz = noise[begin[k]:begin[k] + N]
        x, z = raw[k, :, 0].astype(np.float64), raw[k, :, 2].astype(np.float64)
        turned = np.stack([(x * cs[k, 0] + z * (-cs[k, 1])).astype(np.float32), raw[k, :, 1],
                           (x * cs[k, 1] + z * cs[k, 0]).astype(np.float32), raw[k, :, 3]], 1)
        assert eq(a[k, :, :4], SR.jitter(turned, nz)), k
    assert not eq(a[..., :4], raw[..., :4])


def test_device_generator_batch(dev):
    """8 x 2048 x 6, draws on the device: every output row is a row of its own shape, y untouched by the rotation, x^2 + z^2
    kept within 4 ulp, the jitter inside its clip and shared by the duplicates of a raw row."""
    B, N = 8, 2048
    store, clouds, segs = synthetic_store(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(4)
    d = shapes.draw(store, list(range(B)), N, rotate=True, jitter=True, noise_cols=3, rng=gen)
    assert d.rot.shape == (B, 2) and d.rot.dtype == torch.float64 and d.noise.dtype == torch.float64 and d.choice.shape == (B, N)
    jit, seg, cls = shapes.prepare_shapes(store, None, rng=d)
    rot, seg2, _ = shapes.prepare_shapes(store, None, rng=d._replace(noise=None, noise_begin=None, noise_cols=0))
    assert cls.cpu().tolist() == [b % 16 for b in range(B)] and torch.equal(seg, seg2)
    r, j = rot.cpu().numpy(), jit.cpu().numpy()
    row = r[..., 3].astype(np.int64)
    assert (row == d.choice.cpu().numpy()).all()
    for b in range(B):
        assert row[b].min() >= 0 and row[b].max() < len(clouds[b]) and (r[b, :, 4] == b).all()
        src = clouds[b][row[b]]
        assert eq(r[b, :, 1], src[:, 1]) and eq(r[b, :, 3:], src[:, 3:]) and eq(j[b, :, 3:], src[:, 3:])
        assert (seg[b].cpu().numpy() == segs[b][row[b]]).all()
        want = src[:, 0].astype(np.float64) ** 2 + src[:, 2].astype(np.float64) ** 2
        got = r[b, :, 0].astype(np.float64) ** 2 + r[b, :, 2].astype(np.float64) ** 2
        assert (np.abs(got - want) <= 4 * np.spacing(want.astype(np.float32)).astype(np.float64)).all(), b
        assert not eq(r[b, :, 0], src[:, 0])
        assert len(np.unique(row[b])) > 0.4 * N                  # with replacement out of ~2700: ~53 % distinct expected
    delta = j[..., :3].astype(np.float64) - r[..., :3].astype(np.float64)
    # |noise| <= 0.05 in fp64; the fp32 rounding of the sum of two numbers below 2 adds at most half an ulp of 2
    assert np.abs(delta).max() <= 0.05 + 2.0 ** -23 and np.abs(delta).mean() > 0.005
    first = {}
    shared = 0
    for n in range(N):
        k = int(row[0, n])
        if k in first:
            assert eq(j[0, n], j[0, first[k]])
            shared += 1
        first[k] = n
    assert shared > 100
    # the same through prepare_shapes(rng=generator): another stream, the same invariants of the gather
    out, seg3, _ = shapes.prepare_shapes(store, list(range(B)), N, rotate=False, jitter=False, rng=gen)
    o = out.cpu().numpy()
    for b in range(B):
        rw = o[b, :, 3].astype(np.int64)
        assert eq(o[b], clouds[b][rw]) and (seg3[b].cpu().numpy() == segs[b][rw]).all()


def test_bad_index_is_flagged_and_row_zero_used(dev):
    store, clouds, segs = synthetic_store(dev, B=2, C=6, lo=40, hi=50)
    d = shapes.draw(store, [0, 1], 5, rng="numpy")
    choice = d.choice.clone()
    choice[1, 3] = int(store.row_count[1])                      # one past the end
    choice[0, 0] = -1
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty(2, 5, 6, device=dev)
    lab = torch.empty(2, 5, dtype=torch.int64, device=dev)
    assert launch(store, d, 5, out, lab, bad) == 0 and int(bad) == 0
    assert launch(store, d._replace(choice=choice), 5, out, lab, bad) == 0
    assert int(bad) == 1
    assert eq(out[1, 3], clouds[1][0]) and eq(out[0, 0], clouds[0][0]) and int(lab[1, 3]) == int(segs[1][0])
    c = d.choice.cpu().numpy()
    assert eq(out[1, 4], clouds[1][c[1, 4]]) and eq(out[0, 1], clouds[0][c[0, 1]])
    bad.zero_()                                                  # the identity past the end of a cloud is flagged the same way
    big = torch.empty(2, 64, 6, device=dev)
    assert launch(store, d._replace(choice=None), 64, big, None, bad) == 0 and int(bad) == 1
    assert eq(big[0, :40], clouds[0][:40]) and eq(big[0, 63], clouds[0][0]) and eq(big[1, 50:], np.tile(clouds[1][0], (14, 1)))


def test_out_buffers_and_graph_replay(dev):
    from pointnet12_amd import pointnet_util as U
    store, clouds, segs = synthetic_store(dev, B=4, C=6, lo=500, hi=600)
    np.random.seed(8)
    d1 = shapes.draw(store, [0, 3, 1], 513, rotate=True, jitter=True)
    d2 = shapes.draw(store, [2, 2, 0], 513, rotate=True, jitter=True)
    want1 = [t.clone() for t in shapes.prepare_shapes(store, None, rng=d1)]
    want2 = [t.clone() for t in shapes.prepare_shapes(store, None, rng=d2)]
    bufs = [(torch.zeros(3, 513, 6, device=dev), torch.zeros(3, 513, dtype=torch.int64, device=dev),
             torch.zeros(3, dtype=torch.int64, device=dev)) for _ in range(2)]
    gen0 = U._DATA_GEN[0]
    got = shapes.prepare_shapes(store, None, rng=d1, out=bufs[0])
    assert U._DATA_GEN[0] == gen0 + 1
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, bufs[0]))
    assert eq(bufs[0][0], want1[0]) and torch.equal(bufs[0][1], want1[1]) and torch.equal(bufs[0][2], want1[2])
    with pytest.raises(ValueError):
        shapes.prepare_shapes(store, None, rng=d1, out=(bufs[0][0][:, :512], bufs[0][1], bufs[0][2]))
    for b in bufs:
        for t in b:
            t.zero_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            shapes.prepare_shapes(store, None, rng=d1, out=bufs[0])
            shapes.prepare_shapes(store, None, rng=d2, out=bufs[1])
    torch.cuda.current_stream().wait_stream(side)
    for b in bufs:
        for t in b:
            t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for b, want in zip(bufs, (want1, want2)):
        assert eq(b[0], want[0]) and torch.equal(b[1], want[1]) and torch.equal(b[2], want[2])


# ------------------------------------------------------------------------------------------------ end to end
def test_partseg_training_steps_on_a_shape_store(dev):
    """2 x 1024 from a synthetic store -> PointNet2PartSegMsg_one_hot(50) -> nll_loss -> backward -> Adam, twice."""
    from pointnet12_amd import optim, pointnet2
    from pointnet12_amd.loss import nll_loss
    store, clouds, segs = synthetic_store(dev, B=4, C=6, lo=1100, hi=1300)
    torch.manual_seed(0)
    net = pointnet2.PointNet2PartSegMsg_one_hot(50).to(dev).train()
    opt = optim.Adam(net.parameters(), lr=1e-3)
    np.random.seed(3)
    losses = []
    for ids in ([1, 3], [0, 1]):
        out, seg, cls = shapes.prepare_shapes(store, ids, 1024, rotate=True, jitter=True)
        pts, nrm = out[..., 0:3], out[..., 3:6]
        row = nrm[..., 0].long().cpu().numpy()
        assert all((seg[b].cpu().numpy() == segs[i][row[b]]).all() for b, i in enumerate(ids))
        assert cls.cpu().tolist() == [i % 16 for i in ids]
        one_hot = torch.nn.functional.one_hot(cls, 16).float()
        opt.zero_grad()
        lp = net(pts.transpose(2, 1), nrm.transpose(2, 1), one_hot)
        assert lp.shape == (2, 1024, 50)
        loss = nll_loss(lp.reshape(-1, 50), seg.reshape(-1))
        loss.backward()
        want = -lp.detach().reshape(-1, 50).gather(1, seg.reshape(-1, 1)).double().mean()      # the batch's labels, unchanged
        # (any fp32 summation order of 2048 positive terms stays within 2048 * 2^-24 of the exact mean, relatively)
        assert abs(float(loss.detach()) - float(want)) <= 2048 * 2.0 ** -24 * abs(float(want))
        assert bool(torch.isfinite(loss.detach()))
        for name, p in net.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses))
