"""GPU: HIP geometry kernels (through the C ABI) against golden vectors and the oracle -- bit exact."""
import hashlib

import os

import numpy as np
import pytest
import torch

from conftest import golden
from oracle import geometry as G
from pointnet12_amd import pointnet_util as U
from pointnet12_amd import synthetic as syn

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cu(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def test_fps_golden(dev):
    g = golden("g1_fps.npz")
    for tag in g["cases"]:
        ref = g[tag + "/idx"]
        mine = U.farthest_point_sample(cu(g[tag + "/xyz"], dev), ref.shape[1], cu(g[tag + "/start"], dev))
        assert mine.dtype == torch.int64
        assert (mine.cpu().numpy() == ref).all(), tag


@pytest.mark.parametrize("N,S", [(1, 1), (63, 7), (65, 65), (129, 40), (257, 64), (513, 128), (1025, 100),
                                 (2049, 33), (4097, 64), (8193, 32), (12000, 16), (16385, 8), (20000, 8),
                                 (20481, 8), (24576, 8), (24577, 8), (28672, 12), (28673, 6)])
def test_fps_every_dispatch_bucket_vs_oracle(dev, N, S):
    rng = np.random.default_rng(N)
    xyz = rng.uniform(-1, 1, (3, N, 3)).astype(np.float32)
    xyz[:, N // 2] = xyz[:, 0]                      # duplicates: ties at zero distance
    start = rng.integers(0, N, 3)
    ref = G.farthest_point_sample(xyz, S, start)
    mine = U.farthest_point_sample(cu(xyz, dev), S, cu(start, dev)).cpu().numpy()
    assert (mine == ref).all()


@pytest.mark.parametrize("B,N,S", [(2, 65536, 300), (3, 25000, 257), (1, 100000, 64), (10, 131072, 40)])
def test_fps_cooperative_workgroups_vs_oracle(dev, B, N, S):
    """N > 24 576: one cloud across several cooperating workgroups (cfg5's 65 536-point scans; a 25 000-point
    scan with a partly filled last workgroup; 13 workgroups of 8 points per thread; 16 points per
    thread when 8 would need too many workgroups).  Bit-exact against the oracle, KITTI-shaped duplicates included."""
    pts, _ = syn.kitti_batch(900 + N % 97, B, min(N, 65536))
    xyz = np.ascontiguousarray(pts[:, :3].transpose(0, 2, 1))
    if N > xyz.shape[1]:
        reps = -(-N // xyz.shape[1])
        jitter = np.random.default_rng(N).normal(0, 1e-3, (B, reps * xyz.shape[1], 3)).astype(np.float32)
        xyz = (np.tile(xyz, (1, reps, 1)) + jitter)[:, :N]
    xyz = np.ascontiguousarray(xyz[:, :N])
    start = (np.arange(B) * 9973 + 5) % N
    ref = G.farthest_point_sample(xyz, S, start)
    mine = U.farthest_point_sample(cu(xyz, dev), S, cu(start, dev)).cpu().numpy()
    assert (mine == ref).all()


def test_fps_large_fallback_when_clouds_cannot_be_coscheduled(dev):
    """More clouds than the cooperative plan can keep resident at once: the single-workgroup kernel takes over."""
    rng = np.random.default_rng(3)
    xyz = rng.uniform(-1, 1, (70, 29000, 3)).astype(np.float32)       # 4 workgroups x 70 clouds > 128
    start = rng.integers(0, 29000, 70)
    ref = G.farthest_point_sample(xyz, 6, start)
    assert (U.farthest_point_sample(cu(xyz, dev), 6, cu(start, dev)).cpu().numpy() == ref).all()


def test_fps_full_size_property(dev):
    """B=16 x 4096 -> 1024 (benchmark size): indices distinct until exhaustion, start honoured, oracle-equal."""
    pts, _ = syn.kitti_batch(0, 16, 4096)
    xyz = np.ascontiguousarray(pts[:, :3].transpose(0, 2, 1))
    start = np.arange(16) * 7
    mine = U.farthest_point_sample(cu(xyz, dev), 1024, cu(start, dev)).cpu().numpy()
    assert (mine[:, 0] == start).all()
    assert (mine == G.farthest_point_sample(xyz, 1024, start)).all()
    for b in range(16):
        chosen = xyz[b][mine[b]]
        assert len(np.unique(chosen, axis=0)) == len(chosen)    # never re-picks a location while new ones remain


def test_fps_random_start_uses_cpu_generator(dev):
    xyz = cu(np.random.default_rng(1).uniform(-1, 1, (4, 300, 3)).astype(np.float32), dev)
    torch.manual_seed(77)
    a = U.farthest_point_sample(xyz, 5)
    torch.manual_seed(77)
    expect = torch.randint(0, 300, (4,), dtype=torch.long)
    assert (a[:, 0].cpu() == expect).all()
    with pytest.raises(RuntimeError):
        U.farthest_point_sample(xyz.double(), 5)


def test_ball_query_golden(dev):
    g = golden("g2_ball.npz")
    for tag in g["cases"]:
        fam, rest = tag.split("/")
        r, k = rest[1:].split("_k")
        mine = U.query_ball_point(float(r), int(k), cu(g[fam + "/xyz"], dev), cu(g[fam + "/new_xyz"], dev))
        assert (mine.cpu().numpy() == g[tag]).all(), tag
    for r in (0.1, 0.2, 0.4, 0.8):
        pre = "edge/r%g/" % r
        mine = U.query_ball_point(r, 4, cu(g[pre + "xyz"], dev), cu(g[pre + "new_xyz"], dev))
        assert (mine.cpu().numpy() == g[pre + "idx"]).all()


def test_ball_query_edges(dev):
    xyz = cu(np.random.default_rng(0).uniform(-1, 1, (1, 50, 3)).astype(np.float32), dev)
    far = torch.full((1, 1, 3), 9.0, device=dev)
    idx = U.query_ball_point(0.1, 8, xyz, far)
    assert (idx == 50).all()                                    # empty ball: N everywhere, as the reference
    with pytest.raises(IndexError):
        U.index_points(xyz, idx)                                # and index_points raises on it
    with pytest.raises(RuntimeError):
        U.query_ball_point(0.1, 51, xyz, far)


def test_ball_query_full_size_vs_oracle(dev):
    pts, _ = syn.kitti_batch(3, 4, 4096)
    xyz = np.ascontiguousarray(pts[:, :3].transpose(0, 2, 1))
    new = xyz[:, ::8].copy()
    for r, k in [(0.1, 32), (0.4, 128), (0.8, 128)]:
        mine = U.query_ball_point(r, k, cu(xyz, dev), cu(new, dev)).cpu().numpy()
        assert (mine == G.query_ball_point(r, k, xyz, new)).all()


def test_ball_query_and_three_nn_at_cfg5_size_vs_oracle(dev):
    """BASELINE cfg5: one 65 536-point scan (22.9 % duplicated locations), the MSG x16 level sizes (8192 centroids)."""
    pts, _ = syn.kitti_batch(40, 1, 65536)
    xyz = np.ascontiguousarray(pts[:, :3].transpose(0, 2, 1))
    start = np.array([11])
    fps = U.farthest_point_sample(cu(xyz, dev), 8192, cu(start, dev))
    new = xyz[0][fps.cpu().numpy()[0]][None]
    sub = np.ascontiguousarray(new[:, ::4])                      # 2048 of the centroids keep the scalar oracle in seconds
    for r, k in [(0.1, 32), (0.4, 128)]:
        mine = U.query_ball_point(r, k, cu(xyz, dev), cu(sub, dev)).cpu().numpy()
        assert (mine == G.query_ball_point(r, k, xyz, sub)).all(), (r, k)
    idx, dist, w = U.three_nn(cu(xyz, dev), cu(new, dev))        # fp1 of cfg5: 65 536 targets over 8192 sources
    oi, od = G.three_nn(xyz, new)
    assert (idx.cpu().numpy() == oi).all()
    assert (bits(dist.cpu().numpy()) == bits(od)).all()


def test_square_distance_bits(dev):
    g = golden("g3_sqdist.npz")
    d = U.square_distance(cu(g["new_xyz"], dev), cu(g["xyz"], dev)).cpu().numpy()
    assert hashlib.sha256(bits(d).tobytes()).hexdigest() == str(g["sha256"])


def test_three_nn_interp_golden(dev):
    g = golden("g4_interp.npz")
    for tag in "abc":
        x1, x2, p2 = cu(g[tag + "/xyz1"], dev), cu(g[tag + "/xyz2"], dev), cu(g[tag + "/points2"], dev)
        idx, dist, w = U.three_nn(x1, x2)
        assert (bits(dist.cpu().numpy()) == bits(g[tag + "/dist3"])).all()
        oi, od = G.three_nn(g[tag + "/xyz1"], g[tag + "/xyz2"])
        assert (idx.cpu().numpy() == oi).all()
        assert np.abs(w.cpu().numpy() - G.three_weights(od)).max() <= 1.2e-7
        rows = U._InterpCat.apply(None, p2, idx, w)
        out = rows.view(p2.shape[0], -1, rows.shape[1])[..., :p2.shape[2]].cpu().numpy()
        assert np.abs(out - g[tag + "/interp"]).max() <= 2e-6


def test_index_points_and_grouping(dev):
    rng = np.random.default_rng(5)
    pts = rng.normal(size=(2, 100, 7)).astype(np.float32)
    xyz = rng.normal(size=(2, 100, 3)).astype(np.float32)
    idx = rng.integers(0, 100, (2, 10, 6))
    new = xyz[:, :10].copy()
    assert (U.index_points(cu(pts, dev), cu(idx, dev)).cpu().numpy() == G.index_points(pts, idx)).all()
    assert (U.index_points(cu(pts, dev), cu(idx[:, :, 0], dev)).cpu().numpy() == G.index_points(pts, idx[:, :, 0])).all()
    for first in (True, False):
        rows = U._Group.apply(cu(xyz, dev), cu(pts, dev), cu(new, dev), cu(idx, dev), 10, 6, first)
        ref = G.group(xyz, pts, new, idx, first, ld=12)
        assert (rows.cpu().numpy().reshape(ref.shape) == ref).all()
    # gradient of the gather: scatter-add with repeats
    p = cu(pts, dev).requires_grad_(True)
    U.index_points(p, cu(idx, dev)).sum().backward()
    cnt = np.zeros((2, 100))
    for b in range(2):
        np.add.at(cnt[b], idx[b].ravel(), 1)
    assert np.allclose(p.grad.cpu().numpy(), cnt[..., None].repeat(7, -1))


def test_sample_and_group_api(dev):
    pts, _ = syn.kitti_batch(9, 2, 512)
    xyz = cu(pts[:, :3].transpose(0, 2, 1), dev)
    feat = cu(pts[:, 3:].transpose(0, 2, 1), dev)
    torch.manual_seed(1)
    new_xyz, new_points, grouped_xyz, fps_idx = U.sample_and_group(64, 0.3, 16, xyz, feat, returnfps=True)
    assert new_xyz.shape == (2, 64, 3) and new_points.shape == (2, 64, 16, 9) and grouped_xyz.shape == (2, 64, 16, 3)
    start = fps_idx[:, 0].cpu().numpy()
    oi = G.farthest_point_sample(xyz.cpu().numpy(), 64, start)
    assert (fps_idx.cpu().numpy() == oi).all()
    a, b = U.sample_and_group_all(xyz, feat)
    assert a.shape == (2, 1, 3) and float(a.abs().max()) == 0 and b.shape == (2, 1, 512, 9)
    assert torch.equal(b[:, 0, :, :3], xyz) and torch.equal(b[:, 0, :, 3:], feat)


def test_fps_cooperative_under_graph_replay(dev):
    """The multi-workgroup FPS clears its slot table at every launch; as a graph node that clear must run on every
    replay (a hipMemsetAsync node did not: stale slots let the pollers run ahead of the publishers -- silently wrong
    samples).  Three replays with different start indices, each bit-exact against the oracle."""
    pts, _ = syn.kitti_batch(77, 2, 40000)
    xyz_np = np.ascontiguousarray(pts[:, :3].transpose(0, 2, 1))
    xyz = cu(xyz_np, dev)
    start = torch.zeros(2, dtype=torch.int64, device=dev)
    U.farthest_point_sample(xyz, 200, start)                 # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = U.farthest_point_sample(xyz, 200, start)
    for s0 in ([5, 17], [39999, 0], [123, 20000]):
        start.copy_(torch.tensor(s0))
        g.replay()
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == G.farthest_point_sample(xyz_np, 200, np.array(s0))).all(), s0


@pytest.mark.parametrize("B,M,T", [(3, 5000, 37), (2, 196608, 1024), (2, 40000, 16384), (2, 30000, 20000)])
def test_invert_index_groups_positions_by_target(dev, B, M, T):
    """pn2_invert_index (csrc/scatter.hip): positions of every cloud grouped by the value they point at -- the LDS
    single-pass kernel (T <= 16 384) and the three-pass fallback -- incl. out-of-range entries (dropped, -1 at the end)."""
    rng = np.random.default_rng(B * M + T)
    idx = rng.integers(0, T, (B, M))
    idx[0, ::97] = T + 5                        # out of range: dropped
    idx[1, 5::131] = -1
    members, owners = U._inverse_index(torch.from_numpy(idx).to(dev), T)
    members, owners = members.cpu().numpy(), owners.cpu().numpy()
    for b in range(B):
        valid = (idx[b] >= 0) & (idx[b] < T)
        n = int(valid.sum())
        assert (members[b, n:] == -1).all()
        mem, own = members[b, :n], owners[b, :n]
        assert (np.diff(own) >= 0).all()                         # grouped by target, targets ascending
        assert (idx[b][mem] == own).all()                        # every member points at its owner
        assert np.array_equal(np.sort(mem), np.nonzero(valid)[0])    # each valid position exactly once


def _pruned_case(N, S, kind):
    rng = np.random.default_rng(N + S)
    B = 2
    if kind == "kitti":
        pts, _ = syn.kitti_batch(300 + N % 53, B, N)
        xyz = np.ascontiguousarray(pts[:, :3].transpose(0, 2, 1))
    elif kind == "uniform":
        xyz = rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)
    elif kind == "dups":
        base = rng.uniform(-1, 1, (B, 50, 3)).astype(np.float32)
        xyz = np.stack([base[b][rng.integers(0, 50, N)] for b in range(B)])
    else:
        xyz = np.zeros((B, N, 3), np.float32)
        xyz[:, :, 1] = rng.uniform(-3, 5, (B, N))
        xyz[:, :, 0] = 0.25
    return xyz, rng.integers(0, N, B)


def test_fps_spatially_pruned_kernel_small_clouds_forced():
    """The pruned kernel is slower than the plain one up to N = 8192 and not dispatched there; option FPS_PRUNE = 2 forces it,
    so its 512-thread / 8-points-per-thread instantiations and clouds with EMPTY waves (N far below the capacity) are checked
    against the oracle too.  The library never reads the environment and an option takes effect with the next call: the
    child process is there for the Python binding, which forwards PN2_FPS_PRUNE=2 from ITS environment to pn2_set_option
    once, when it loads the library (_lib.forward_env_options) -- the way A/B runs select a route."""
    import subprocess
    import sys
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import numpy as np, torch\n"
            "import test_geometry_gpu as T\n"
            "from oracle import geometry as G\n"
            "from pointnet12_amd import pointnet_util as U\n"
            "dev = torch.device('cuda:0')\n"
            "for N, S in [(2049, 100), (5000, 700), (8192, 300), (12000, 200)]:\n"
            "    for kind in ('kitti', 'uniform', 'dups', 'flat'):\n"
            "        xyz, start = T._pruned_case(N, S, kind)\n"
            "        ref = G.farthest_point_sample(xyz, S, start)\n"
            "        mine = U.farthest_point_sample(T.cu(xyz, dev), S, T.cu(start, dev)).cpu().numpy()\n"
            "        assert (mine == ref).all(), (N, S, kind, np.argwhere(mine != ref)[:3])\n"
            "print('PRUNED-SMALL-OK')\n") % (os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=dict(os.environ, PN2_FPS_PRUNE="2"))
    assert p.returncode == 0 and "PRUNED-SMALL-OK" in p.stdout, (p.stdout[-500:], p.stderr[-2000:])


@pytest.mark.parametrize("N,S", [(8193, 300), (12000, 200), (16384, 128), (20000, 200), (22000, 100),
                                 (24576, 100), (25000, 300), (25600, 90), (26624, 70), (28672, 100)])
@pytest.mark.parametrize("kind", ["kitti", "uniform", "dups", "flat"])
def test_fps_spatially_pruned_kernel_vs_oracle(dev, N, S, kind):
    """fps_pruned_kernel (2048 < N <= 28 672, npoint >= 64): points sorted by Morton cell, a wave whose bounding box is farther
    from the new sample than its largest running distance skips the update.  The skip must be EXACT: bit-equal indices against
    the oracle on KITTI-shaped clouds (9-23 % duplicate points: equal distances inside one thread take the slow tie path),
    a uniform cube (no spatial structure to prune on early), a cloud of 50 distinct points repeated (exhaustion: every
    distance 0, then index 0 forever) and a degenerate flat cloud (zero extent in z, all x equal)."""
    xyz, start = _pruned_case(N, S, kind)
    ref = G.farthest_point_sample(xyz, S, start)
    mine = U.farthest_point_sample(cu(xyz, dev), S, cu(start, dev)).cpu().numpy()
    assert (mine == ref).all(), (np.argwhere(mine != ref)[:3], kind)


@pytest.mark.parametrize("B,N,S", [(16, 4096, 512), (2, 1024, 512), (8, 2048, 256)])
def test_fps_beside_the_pooled_split_forward_is_index_exact(dev, B, N, S):
    """Round 6 (HISTORY.md: "pn2_fps beside the pooled bf16-split forward"): the captured training step runs the next batch's sampling on
    a side stream while the main stream runs the MLPs.  Co-resident with the pooled split_nt forward, pn2_fps used to return a different
    sample list in 4 .. 100 % of the launches: its packed distance arithmetic read the winner's y through the HIGH half of a register pair
    (v_pk_add_f32 ... op_sel:[0,1]), a form that is wrong in lanes 48..63 beside bf16 MFMAs on this hardware (PN2_OPAQUE in pn2_common.h).  Here: the same launch on a side stream beside that kernel, 40 times, against the oracle's list -- bit for bit."""
    from pointnet12_amd import _lib
    from pointnet12_amd._lib import ptr as p

    lib = _lib.load()
    pts, _ = syn.kitti_batch(0, B, N)
    xyz_np = np.ascontiguousarray(pts[:, :3, :].transpose(0, 2, 1))
    xyz = cu(xyz_np, dev)
    P = 1 << 18
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(P, 96, device=dev, generator=g)
    W = torch.randn(128, 96, device=dev, generator=g)
    bias = torch.randn(128, device=dev, generator=g)
    Y = torch.empty(P, 128, device=dev)
    aff = torch.zeros(4 * 96, device=dev)
    aff[96:192] = 1
    aff[288:] = 1
    stats = torch.zeros(8 * 2 * 128, device=dev, dtype=torch.float64)
    ws = torch.zeros(2 * (P // 128) * 128, device=dev)
    main_s = torch.cuda.current_stream().cuda_stream

    def pooled_forward():
        rc = lib.pn2_conv1x1_fwd_pool(p(X), 96, p(aff), p(W), 96, p(bias), p(Y), 128, P, 96, 128, p(stats), 128, p(bias), p(ws), None, main_s)
        assert rc == 0
        assert b"split_nt_kernel" in (lib.pn2_last_kernel() or b""), "this test is about the bf16-split pooled forward"

    side = torch.cuda.Stream(device=dev)
    rng = np.random.default_rng(1)
    differ = 0
    for wg2 in (1, 0):                              # two workgroups per CU (the default) and one (pn2_fps finds room on every CU)
        _lib.set_option("PN2_SPLIT_WG2", wg2)
        try:
            for _ in range(20):
                start_np = rng.integers(0, N, B)
                ref = G.farthest_point_sample(xyz_np, S, start_np)
                start = cu(start_np, dev)
                torch.cuda.synchronize()
                side.wait_stream(torch.cuda.current_stream())
                pooled_forward()
                with torch.cuda.stream(side):
                    mine = U.farthest_point_sample(xyz, S, start)
                pooled_forward()
                pooled_forward()
                torch.cuda.synchronize()
                differ += int(not (mine.cpu().numpy() == ref).all())
        finally:
            _lib.set_option("PN2_SPLIT_WG2", 1)
    assert differ == 0, "%d of 40 pn2_fps launches beside the pooled split forward differ from the oracle" % differ


def test_ball_query_and_three_nn_beside_the_pooled_split_forward_are_index_exact(dev):
    """The rest of the captured step's geometry branch under the same co-residency as the test above (both kernels read LDS and compute
    with packed fp32 operations): 20 launches each on a side stream beside the pooled split_nt forward equal the launch alone."""
    from pointnet12_amd import _lib
    from pointnet12_amd._lib import ptr as p

    lib = _lib.load()
    B, N, S = 16, 4096, 1024
    pts, _ = syn.kitti_batch(0, B, N)
    xyz = cu(np.ascontiguousarray(pts[:, :3, :].transpose(0, 2, 1)), dev)
    new_xyz = xyz[:, :S].contiguous()
    P = 1 << 18
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(P, 96, device=dev, generator=g)
    W = torch.randn(128, 96, device=dev, generator=g)
    bias = torch.randn(128, device=dev, generator=g)
    Y = torch.empty(P, 128, device=dev)
    aff = torch.zeros(4 * 96, device=dev)
    aff[96:192] = 1
    aff[288:] = 1
    stats = torch.zeros(8 * 2 * 128, device=dev, dtype=torch.float64)
    ws = torch.zeros(2 * (P // 128) * 128, device=dev)
    main_s = torch.cuda.current_stream().cuda_stream

    def pooled_forward():
        assert lib.pn2_conv1x1_fwd_pool(p(X), 96, p(aff), p(W), 96, p(bias), p(Y), 128, P, 96, 128, p(stats), 128, p(bias), p(ws), None, main_s) == 0

    ref_bq = U.query_ball_point(0.2, 32, xyz, new_xyz)
    ref_i, ref_d = U.three_nn(xyz, new_xyz)[:2]
    side = torch.cuda.Stream(device=dev)
    differ = 0
    for wg2 in (1, 0):
        _lib.set_option("PN2_SPLIT_WG2", wg2)
        try:
            for _ in range(10):
                torch.cuda.synchronize()
                side.wait_stream(torch.cuda.current_stream())
                pooled_forward()
                with torch.cuda.stream(side):
                    bq = U.query_ball_point(0.2, 32, xyz, new_xyz)
                    i, d = U.three_nn(xyz, new_xyz)[:2]
                pooled_forward()
                pooled_forward()
                torch.cuda.synchronize()
                differ += int(not (torch.equal(bq, ref_bq) and torch.equal(i, ref_i) and torch.equal(d, ref_d)))
        finally:
            _lib.set_option("PN2_SPLIT_WG2", 1)
    assert differ == 0, "%d of 20 launches beside the pooled split forward differ from the launch alone" % differ
