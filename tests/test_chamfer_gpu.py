"""GPU: the Chamfer kernels (csrc/chamfer.hip through pointnet12_amd/chamfer.py) against fp64 (tests/chamfer_ref.py, tied to the
reference by tests/test_chamfer_cpu.py) and, on the recorded cases, against the reference's own numbers (g15_chamfer.npz).

Bounds (chamfer_ref.py states and derives them): per point |dist - d64| <= 2e-6 d64 and dist == 0 exactly where d64 == 0; value
5e-6 relative; dp1 3e-6 |g|/B per component; dp2 4e-6 (|g|/B) max(1, c), c = queries that chose the candidate; zero rows exactly
zero.  On the recorded cases idx must equal the fp64 arg-min EVERYWHERE (the generator asserted a relative gap >= 1e-5 between the
nearest and the next distance).  On the seeded sweep every chosen candidate must be within (1 + 4e-6) of the nearest in fp64, dist
is held against the chosen candidate's fp64 distance and the gradients against the fp64 formulas at the kernel's own idx.
Against the REFERENCE's recorded fp32 numbers the bound is the sum of the two bounds against fp64 (both sides were held to them:
the reference's by test_chamfer_cpu.py)."""
import numpy as np
import pytest
import torch

from conftest import golden
import chamfer_ref as C

pytestmark = pytest.mark.gpu


def _mod():
    from pointnet12_amd import chamfer as M
    return M


def run(p1, p2, g, fn=None):
    """-> dist, idx, value, dp1, dp2 of the HIP path for upstream scalar g."""
    M = _mod()
    a, b = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
    v = (fn or M.chamfer_batch)(a, b)
    assert v.shape == () and v.dtype == torch.float32 and v.device == p1.device
    v.backward(torch.tensor(float(g), device=p1.device))
    dist, idx = M.nearest_neighbor(p1, p2)
    assert dist.shape == p1.shape[:2] and idx.shape == p1.shape[:2] and dist.dtype == torch.float32 and idx.dtype == torch.int64
    assert not dist.requires_grad
    return dist, idx, v.detach(), a.grad, b.grad


def seeded(seed, B, N, M, D, dev):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(B, N, D, generator=gen) * 2 - 1).to(dev), (torch.rand(B, M, D, generator=gen) * 2 - 1).to(dev)


def test_recorded_cases_against_fp64_and_the_reference(dev):
    g = golden("g15_chamfer.npz")
    M = _mod()
    for c in [str(c) for c in g["cases"]]:
        p1, p2 = torch.from_numpy(g[c + "/p1"]).to(dev), torch.from_numpy(g[c + "/p2"]).to(dev)
        gr, B = float(g[c + "/g"]), p1.shape[0]
        fn = getattr(M, str(g[c + "/fn"]))
        dist, idx, v, dp1, dp2 = run(p1, p2, gr, fn)
        want = torch.from_numpy(g[c + "/argmin"].astype(np.int64)).to(dev)
        fig = C.check_against(p1, p2, gr, dist, idx, v, dp1, dp2, exact_idx=want, what=c)
        # the reference's recorded numbers
        ref_v = float(g[c + "/value"])
        unit = abs(gr) / B
        _, _, count = C.gradients(p1, p2, want, gr)
        fig["ref_value_rel"] = abs(float(v) - ref_v) / abs(ref_v)
        fig["ref_dp1/unit"] = float((dp1.double().cpu() - torch.from_numpy(g[c + "/dp1"]).double()).abs().max()) / unit
        rel2 = (dp2.double().cpu() - torch.from_numpy(g[c + "/dp2"]).double()).abs().amax(dim=2) / (unit * count.cpu().clamp(min=1))
        fig["ref_dp2/(unit*max(1,c))"] = float(rel2.max())
        print(c, fig)
        assert fig["ref_value_rel"] <= 2 * C.VALUE_REL, c
        assert fig["ref_dp1/unit"] <= 2 * C.DP1_ABS, c
        assert fig["ref_dp2/(unit*max(1,c))"] <= 2 * C.DP2_ABS, c
    assert "%.4f" % float(run(torch.from_numpy(g["main/p1"]).to(dev), torch.from_numpy(g["main/p2"]).to(dev), 1.0)[2]) == "11.6073"


SWEEP = [(1, 1, 1), (3, 1, 1000), (3, 1000, 1), (16, 63, 65), (3, 64, 64), (16, 65, 63), (16, 1000, 1000), (3, 4096, 4096),
         (1, 2048, 2048), (3, 8191, 1000), (3, 4096, 8191), (1, 8191, 8191), (1, 65536, 8191), (1, 8191, 65536), (1, 65536, 65536)]


@pytest.mark.parametrize("B,N,M", SWEEP)
def test_shape_sweep_against_fp64(dev, B, N, M):
    p1, p2 = seeded(1000 * B + N + 7 * M, B, N, M, 3, dev)
    dist, idx, v, dp1, dp2 = run(p1, p2, -0.625)
    fig = C.check_against(p1, p2, -0.625, dist, idx, v, dp1, dp2, what="%dx%dx%d" % (B, N, M))
    _, i64 = C.nearest(p1, p2)
    fig["argmin_mismatches"] = int((i64 != idx).sum())
    print((B, N, M), fig)


@pytest.mark.parametrize("D", list(range(1, 17)))
def test_every_point_dimension(dev, D):
    for B, N, M in ((2, 300, 257), (1, 1111, 77)):
        p1, p2 = seeded(50 + D, B, N, M, D, dev)
        dist, idx, v, dp1, dp2 = run(p1, p2, 1.5)
        print(D, (B, N, M), C.check_against(p1, p2, 1.5, dist, idx, v, dp1, dp2, what="D=%d" % D))


def test_unsupported_dimension_and_dtype_are_refused(dev):
    from pointnet12_amd import _lib
    M = _mod()
    p1, p2 = seeded(1, 2, 40, 30, 17, dev)
    for fn in (M.chamfer_batch, M.nearest_neighbor, M.chamfer_symmetric):
        with pytest.raises(_lib.Pn2Error, match="D = 17"):
            fn(p1, p2)
    with pytest.raises(RuntimeError, match="float32"):
        M.chamfer_batch(p1[:, :, :3].double(), p2[:, :, :3].double())
    with pytest.raises(IndexError):
        M.chamfer_batch(p1, p2[:, :0])
    assert float(M.chamfer_batch(p1[:, :0, :3], p2[:, :, :3])) == 0.0          # N == 0: the reference returns 0


def test_noncontiguous_inputs_and_the_other_entry_points(dev):
    M = _mod()
    gen = torch.Generator(device="cpu").manual_seed(9)
    a = (torch.rand(3, 3, 700, generator=gen) * 2 - 1).to(dev)                 # [B, D, N], handed over transposed
    b = (torch.rand(3, 3, 450, generator=gen) * 2 - 1).to(dev)
    at, bt = a.requires_grad_(True).transpose(1, 2), b.requires_grad_(True).transpose(1, 2)
    assert not at.is_contiguous()
    v = M.chamfer_batch(at, bt)
    v.backward(torch.tensor(2.0, device=dev))
    p1, p2 = a.detach().transpose(1, 2).contiguous(), b.detach().transpose(1, 2).contiguous()
    dist, idx = M.nearest_neighbor(at, bt)
    C.check_against(p1, p2, 2.0, dist, idx, v.detach(), a.grad.transpose(1, 2), b.grad.transpose(1, 2), what="transposed")
    assert torch.equal(v.detach(), M.chamfer_batch(p1, p2))
    # chamfer_symmetric = the two directions; chamfer_non_batch = the sum of one cloud
    s = M.chamfer_symmetric(p1, p2)
    assert torch.equal(s, M.chamfer_batch(p1, p2) + M.chamfer_batch(p2, p1))
    d12, _ = C.nearest(p1, p2)
    d21, _ = C.nearest(p2, p1)
    want = float(C.value(d12) + C.value(d21))
    assert abs(float(s) - want) <= C.VALUE_REL * want
    one = M.chamfer_non_batch(p1[:1], p2[:1])
    assert abs(float(one) - float(d12[0].sum())) <= C.VALUE_REL * float(d12[0].sum())
    # only one input needs a gradient
    q = p1.clone().requires_grad_(True)
    M.chamfer_batch(q, p2).backward()
    r = p2.clone().requires_grad_(True)
    M.chamfer_batch(p1, r).backward()
    C.check_against(p1, p2, 1.0, None, idx, None, q.grad, r.grad, what="single-sided")


@pytest.mark.parametrize("B,N,M", [(16, 4096, 1024), (1, 2048, 2048), (2, 65536, 3000)])
def test_run_to_run_identical(dev, B, N, M):
    p1, p2 = seeded(3, B, N, M, 3, dev)
    first = run(p1, p2, 0.5)
    second = run(p1, p2, 0.5)
    for name, x, y in zip(("dist", "idx", "value", "dp1"), first[:4], second[:4]):
        assert torch.equal(x, y), name
    unit = 0.5 / B
    _, _, count = C.gradients(p1, p2, first[1], 0.5)
    assert bool(((first[4] - second[4]).abs().amax(dim=2).double() <= C.DP2_ABS * unit * count.clamp(min=1)).all())


def test_nothing_of_size_n_times_m_is_allocated(dev):
    B, N, M = 16, 4096, 4096
    p1, p2 = seeded(4, B, N, M, 3, dev)
    Mod = _mod()
    a, b = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
    Mod.chamfer_batch(a, b).backward()                   # warm-up: code objects, the zero arena
    a.grad = b.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    Mod.chamfer_batch(a, b).backward()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated(dev) - before
    print("peak growth over forward + backward: %d bytes (one fp32 [B,N,M] is %d)" % (grown, B * N * M * 4))
    assert grown < B * N * M * 4


def test_forward_and_backward_under_graph_capture(dev):
    M = _mod()
    B, N, Mc = 4, 3000, 1700
    inputs = [seeded(20 + i, B, N, Mc, 3, dev) for i in range(3)]
    s1 = inputs[0][0].clone().requires_grad_(True)
    s2 = inputs[0][1].clone().requires_grad_(True)
    gs = torch.tensor(0.75, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):                                # warm-up on the capture stream
            v = M.chamfer_batch(s1, s2)
            v.backward(gs)
            s1.grad = s2.grad = None
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            v = M.chamfer_batch(s1, s2)
            v.backward(gs)
            dist, idx = M.nearest_neighbor(s1, s2)
    torch.cuda.current_stream(dev).wait_stream(side)
    for i in (1, 2):
        p1, p2 = inputs[i]
        with torch.no_grad():
            s1.copy_(p1)
            s2.copy_(p2)
            gs.fill_(0.75 * i)
        graph.replay()
        torch.cuda.synchronize()
        e_dist, e_idx, e_v, e_dp1, e_dp2 = run(p1, p2, 0.75 * i)
        assert torch.equal(dist, e_dist) and torch.equal(idx, e_idx) and torch.equal(v.detach(), e_v), i
        assert torch.equal(s1.grad, e_dp1), i
        _, _, count = C.gradients(p1, p2, e_idx, 0.75 * i)
        unit = 0.75 * i / B
        assert bool(((s2.grad - e_dp2).abs().amax(dim=2).double() <= C.DP2_ABS * unit * count.clamp(min=1)).all()), i
        C.check_against(p1, p2, 0.75 * i, dist, idx, v.detach(), s1.grad, s2.grad, what="replay %d" % i)


@pytest.mark.parametrize("B,N,M", [(16, 4096, 4096), (16, 4096, 1024)])
def test_not_slower_than_the_stock_formulation(dev, B, N, M):
    """Forward + backward, HIP against stock torch fp32 in the formulation it replaces, same process, same card: warm-up, then
    the median of 25 event-timed runs each, interleaved."""
    Mod = _mod()
    p1, p2 = seeded(5, B, N, M, 3, dev)
    a, b = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)

    def hip():
        a.grad = b.grad = None
        Mod.chamfer_batch(a, b).backward()

    def stock():
        a.grad = b.grad = None
        C.stock_chamfer(a, b).backward()

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e)

    for _ in range(3):
        hip()
        stock()
    torch.cuda.synchronize()
    t_hip, t_stock = [], []
    for _ in range(25):
        t_hip.append(timed(hip))
        t_stock.append(timed(stock))
    m_hip, m_stock = float(np.median(t_hip)), float(np.median(t_stock))
    print("%dx%dx%dx3 forward+backward: HIP %.3f ms, stock torch %.3f ms (medians of 25)" % (B, N, M, m_hip, m_stock))
    assert m_hip <= m_stock
