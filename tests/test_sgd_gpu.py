"""GPU: pn2_sgd_step / optim.SGD against torch.optim.SGD on CPU tensors fed the same gradients, on raw fp32 bits (the kernel
writes ATen's roundings with fmaf: tests/sgd_ref.py, tests/test_sgd_cpu.py), through the C ABI and through the optimiser."""
import numpy as np
import pytest
import torch

import sgd_ref as R
from pointnet12_amd import _lib, optim

pytestmark = pytest.mark.gpu

EINVAL = -1
IDS = [",".join("%s=%s" % kv for kv in o.items()) or "plain" for o in R.OPTION_SETS]


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def flat(tensors):
    return torch.cat([t.detach().reshape(-1) for t in tensors]).cpu().numpy()


def same_bits(mine, ref, what):
    a, b = bits(mine), bits(ref)
    differing = int((a != b).sum())
    assert differing == 0, "%s: %d of %d elements differ from torch, max |diff| %g" % (
        what, differing, a.size, np.abs(a.view(np.float32).astype(np.float64) - b.view(np.float32)).max())


def draw(shapes, gen=None):
    """Gradients as in test_adam_matches_torch_and_oracle: randn times 10^k, k in [-4, 0]."""
    return [torch.randn(s, generator=gen) * 10.0 ** float(torch.randint(-4, 1, (1,), generator=gen)) for s in shapes]


def feed(ref_p, my_p, grads):
    for p, q, gr in zip(ref_p, my_p, grads):
        p.grad = gr.clone()
        q.grad.copy_(gr)


def buffers(opt, params):
    return [opt.state[p]["momentum_buffer"] for p in params]


# ----------------------------------------------------------------------------------------------- 1. ragged sizes
@pytest.mark.parametrize("sizes", [[(1,)], [(7,), (3, 5), (1,)], [(1027,), (64, 9, 1, 1), (2,)]],
                         ids=["tail_only", "23", "1605"])
@pytest.mark.parametrize("opts", R.OPTION_SETS, ids=IDS)
def test_sgd_matches_torch_bit_for_bit(dev, opts, sizes):
    """Parameters and momentum buffers after every one of 8 steps, StepLR(3, 0.5) on both (semseg.py:113)."""
    torch.manual_seed(11)
    init = [torch.randn(s) for s in sizes]
    ref_p = [torch.nn.Parameter(t.clone()) for t in init]
    my_p = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    ref = torch.optim.SGD(ref_p, lr=0.01, **opts)
    mine = optim.SGD(my_p, lr=0.01, **opts)
    s_ref = torch.optim.lr_scheduler.StepLR(ref, step_size=3, gamma=0.5)
    s_mine = torch.optim.lr_scheduler.StepLR(mine, step_size=3, gamma=0.5)
    for t in range(1, 9):
        ref.zero_grad()
        mine.zero_grad()
        feed(ref_p, my_p, draw(sizes))
        assert mine.param_groups[0]["lr"] == ref.param_groups[0]["lr"]
        ref.step()
        mine.step()
        s_ref.step()
        s_mine.step()
        same_bits(flat(my_p), flat(ref_p), "parameters, step %d" % t)
        if opts.get("momentum", 0) != 0:
            same_bits(flat(buffers(mine, my_p)), flat(buffers(ref, ref_p)), "momentum buffers, step %d" % t)
    assert mine.steps_taken() == [8]
    for p, q in zip(ref_p, my_p):
        assert q.shape == p.shape and q.is_contiguous()


# ----------------------------------------------------------------------------------------------- 2. through the C ABI
def torch_two_steps(p0, grads, **kw):
    """torch.optim.SGD on CPU: [(param, buffer) after step 1, after step 2]."""
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.SGD([p], **kw)
    out = []
    for g in grads:
        p.grad = g.clone()
        opt.step()
        out.append((p.detach().clone(), opt.state[p]["momentum_buffer"].clone()))
    return out


def test_sgd_step_grid_stride_loop(dev):
    """More float4s than the 8 192 workgroups x 256 threads cover in one trip, plus a tail of 5 - 4 = 1 element after the last
    whole float4: one step from t = 1 (the buffer is written, not read) and one from t = 2."""
    n = 8192 * 256 * 4 + 5
    gen = torch.Generator().manual_seed(3)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 1e-2]
    kw = dict(lr=0.01, momentum=0.9, weight_decay=1e-4)
    want = torch_two_steps(p0, grads, **kw)
    lib = _lib.load()
    p, g = p0.to(dev), torch.empty(n, device=dev)
    buf = torch.full((n,), 7.0, device=dev)                     # step 1 must overwrite it, not blend it in
    for t, (gr, (wp, wb)) in enumerate(zip(grads, want), 1):
        g.copy_(gr)
        assert lib.pn2_sgd_step(p.data_ptr(), g.data_ptr(), buf.data_ptr(), n, 0.01, 0.9, 0.0, 1e-4, 0, 0, t, None, None,
                                0, _lib.stream()) == 0
        same_bits(p, wp, "parameters, step %d" % t)
        same_bits(buf, wb, "momentum buffer, step %d" % t)
        same_bits(g, gr, "gradient (zero_grad == 0 leaves it), step %d" % t)


def test_sgd_step_unaligned_scalar_kernel(dev):
    """All pointers one float off a 16-byte boundary: the scalar kernel.  The element in front of each range and the one behind
    it come back unchanged."""
    n = 1030
    gen = torch.Generator().manual_seed(4)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 1e-2]
    want = torch_two_steps(p0, grads, lr=0.01, momentum=0.9, weight_decay=1e-4)
    lib = _lib.load()
    guard = [11.0, 22.0, 33.0]
    hold = [torch.full((n + 2,), v, device=dev) for v in guard]
    p, g, buf = (h[1:n + 1] for h in hold)
    assert all(h.data_ptr() % 16 == 0 for h in hold) and p.data_ptr() % 16 == 4
    p.copy_(p0)
    for t, (gr, (wp, wb)) in enumerate(zip(grads, want), 1):
        g.copy_(gr)
        assert lib.pn2_sgd_step(p.data_ptr(), g.data_ptr(), buf.data_ptr(), n, 0.01, 0.9, 0.0, 1e-4, 0, 0, t, None, None,
                                1, _lib.stream()) == 0
        same_bits(p, wp, "parameters, step %d" % t)
        same_bits(buf, wb, "momentum buffer, step %d" % t)
        assert float(g.abs().max()) == 0                        # zero_grad == 1 cleared exactly the range
        for h, v in zip(hold, guard):
            assert float(h[0]) == v and float(h[n + 1]) == v


# ----------------------------------------------------------------------------------------------- 3. momentum == 0
def test_sgd_without_momentum_has_no_buffer(dev):
    torch.manual_seed(6)
    sizes = [(129,), (5, 3)]
    init = [torch.randn(s) for s in sizes]
    ref_p = [torch.nn.Parameter(t.clone()) for t in init]
    my_p = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    ref = torch.optim.SGD(ref_p, lr=0.05, weight_decay=1e-4)
    mine = optim.SGD(my_p, lr=0.05, weight_decay=1e-4)
    assert mine._flat[0]["buf"] is None
    for t in range(1, 4):
        mine.zero_grad()
        feed(ref_p, my_p, draw(sizes))
        ref.step()
        with _lib.call_profile() as calls:
            mine.step()
        assert [c[0] for c in calls] == ["pn2_sgd_step"] and calls[0][1][2] is None       # one launch, a NULL buffer
        same_bits(flat(my_p), flat(ref_p), "parameters, step %d" % t)
    assert mine._flat[0]["buf"] is None and mine.state_dict()["state"] == {}
    assert mine.state_dict()["param_groups"][0]["steps_taken"] == 3


# ----------------------------------------------------------------------------------------------- 4. bad arguments
def test_sgd_step_argument_checks(dev):
    lib = _lib.load()
    p0 = torch.randn(64)
    p, g, buf = p0.to(dev), torch.ones(64, device=dev), torch.zeros(64, device=dev)
    a = (p.data_ptr(), g.data_ptr(), buf.data_ptr())
    st = _lib.stream()
    assert lib.pn2_sgd_step(*a, 64, 0.01, 0.9, 0.1, 0.0, 1, 0, 1, None, None, 1, st) == EINVAL      # nesterov with dampening
    assert lib.pn2_sgd_step(*a, 64, 0.01, 0.0, 0.0, 0.0, 1, 0, 1, None, None, 1, st) == EINVAL      # nesterov without momentum
    assert lib.pn2_sgd_step(a[0], a[1], None, 64, 0.01, 0.9, 0.0, 0.0, 0, 0, 1, None, None, 1, st) == EINVAL
    assert lib.pn2_sgd_step(*a, 0, 0.01, 0.9, 0.0, 0.0, 0, 0, 1, None, None, 1, st) == EINVAL
    for lr, mu, wd in ((-0.01, 0.9, 0.0), (0.01, -0.9, 0.0), (0.01, 0.9, -1e-4)):
        assert lib.pn2_sgd_step(*a, 64, lr, mu, 0.0, wd, 0, 0, 1, None, None, 1, st) == EINVAL
    torch.cuda.synchronize()
    # without a launch: nothing moved, the gradient was not cleared
    same_bits(p, p0, "parameters")
    assert float(g.min()) == 1 and float(buf.abs().max()) == 0


# ----------------------------------------------------------------------------------------------- 5. checkpoints
def test_sgd_state_dict_round_trips_with_torch(dev):
    torch.manual_seed(2)
    sizes = [(33, 5), (33,)]
    init = [torch.randn(s) for s in sizes]
    kw = dict(lr=0.01, momentum=0.9, dampening=0.1, weight_decay=1e-4)
    a = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    ta = torch.optim.SGD(a, **kw)
    for _ in range(3):
        for p in a:
            p.grad = torch.randn_like(p)
        ta.step()
    b = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    mine = optim.SGD(b, **kw)
    sd0 = mine.state_dict()
    assert [s["momentum_buffer"] for s in sd0["state"].values()] == [None, None]           # before the first step
    assert sd0["param_groups"][0]["steps_taken"] == 0
    c = [torch.nn.Parameter(p.detach().cpu().clone()) for p in a]                          # the yardstick: CPU tensors
    tc = torch.optim.SGD(c, **kw)
    tc.load_state_dict(ta.state_dict())
    with torch.no_grad():
        for p, q in zip(a, b):
            q.copy_(p)
    mine.load_state_dict(ta.state_dict())                                                  # resume a torch.optim.SGD checkpoint
    assert mine.steps_taken() == [1]                                                       # past the first step: max(0, 1)
    same_bits(flat(buffers(mine, b)), flat(buffers(ta, a)), "loaded buffers")
    for t in range(2):
        grads = draw(sizes)
        mine.zero_grad()
        feed(c, b, grads)
        for p, gr in zip(a, grads):
            p.grad = gr.to(dev)
        tc.step()
        ta.step()
        mine.step()
        # a first step would have overwritten the loaded buffers with the gradient
        same_bits(flat(b), flat(c), "parameters, step %d after the load" % t)
        same_bits(flat(buffers(mine, b)), flat(buffers(tc, c)), "buffers, step %d after the load" % t)
    same_bits(flat(b), flat(a), "parameters against torch.optim.SGD on the device")
    # and back: a fresh torch.optim.SGD takes this class's state dict
    d = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    tb = torch.optim.SGD(d, **kw)
    tb.load_state_dict(mine.state_dict())
    same_bits(flat(buffers(tb, d)), flat(buffers(mine, b)), "buffers loaded into torch")
    # save and reload of this class resumes exactly
    e = [torch.nn.Parameter(q.detach().clone()) for q in b]
    again = optim.SGD(e, **kw)
    again.load_state_dict(mine.state_dict())
    assert again.steps_taken() == mine.steps_taken() == [3]
    grads = draw(sizes)
    mine.zero_grad()
    again.zero_grad()
    feed(c, b, grads)
    feed(c, e, grads)
    tc.step()
    mine.step()
    again.step()
    same_bits(flat(e), flat(b), "resumed parameters")
    same_bits(flat(e), flat(c), "resumed parameters against torch")
    same_bits(flat(buffers(again, e)), flat(buffers(tc, c)), "resumed buffers against torch")


# ----------------------------------------------------------------------------------------------- 6. graph replay
def test_sgd_device_step_replays_from_a_graph(dev):
    """device_step: t and lr live in HBM, the captured launch advances t itself; fused_zero_grad clears the bucket."""
    torch.manual_seed(5)
    init = [torch.randn(257, 3), torch.randn(1025)]
    kw = dict(lr=0.01, momentum=0.9, dampening=0.1, weight_decay=1e-4)
    a = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    b = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    host = optim.SGD(a, **kw)
    graphed = optim.SGD(b, device_step=True, fused_zero_grad=True, **kw)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            graphed.step()
    torch.cuda.synchronize()
    # the capture itself launches nothing: parameters and the step cell are untouched
    assert graphed.steps_taken() == [0]
    same_bits(flat(b), flat(a), "parameters after the capture")
    for t in range(1, 8):
        grads = [torch.randn_like(p) * 0.1 for p in a]
        host.zero_grad()
        for p, q, gr in zip(a, b, grads):
            p.grad.copy_(gr)
            assert float(q.grad.abs().max()) == 0               # cleared by the previous fused step
            q.grad.copy_(gr)
        if t == 4:
            host.param_groups[0]["lr"] = graphed.param_groups[0]["lr"] = 2.5e-3
            graphed.sync_lr()
        host.step()
        graph.replay()
        torch.cuda.synchronize()
        assert graphed.steps_taken() == [t]
        same_bits(flat(b), flat(a), "parameters, replay %d" % t)       # dampening would show a replay that took t for 1
        same_bits(graphed._flat[0]["buf"], host._flat[0]["buf"], "momentum buffer, replay %d" % t)
    assert int(graphed._flat[0]["step_dev"][1]) == 0                # ticket re-armed
    assert float(graphed._flat[0]["g"].abs().max()) == 0            # the fused zero-grad left the bucket clear
    sd = graphed.state_dict()
    assert sd["param_groups"][0]["steps_taken"] == 7 and sd["state"][0]["momentum_buffer"] is not None
    # host-side step count and lr cannot be captured
    plain = optim.SGD([torch.nn.Parameter(torch.randn(9, device=dev))], **kw)
    g2, cell = torch.cuda.CUDAGraph(), torch.zeros(1, device=dev)
    before = plain._flat[0]["p"].cpu().numpy().copy()
    torch.cuda.synchronize()
    with pytest.raises(_lib.Pn2Error, match="device_step=True"):
        with torch.cuda.stream(side):
            with torch.cuda.graph(g2, stream=side):
                cell.add_(1)                                        # (the capture that ends on the error is not an empty one)
                plain.step()
    torch.cuda.synchronize()
    assert plain.steps_taken() == [0] and (bits(plain._flat[0]["p"]) == bits(before)).all()


# ----------------------------------------------------------------------------------------------- 7. network wiring
def test_sgd_keeps_the_network_wired(dev):
    """Re-pointing the parameters into the flat buffer must not change the network, gradients must land in the
    shared bucket, and three optimiser steps must lower the loss on a fixed batch."""
    from pointnet12_amd import pointnet2, pointnet_util, synthetic as syn
    from pointnet12_amd.loss import nll_loss
    from pointnet12_amd.parallel import FlatGradBucket
    torch.manual_seed(0)
    net = pointnet2.PointNet2SemSeg(13, feature_dims=1).to(dev)
    pts_np, lab_np = syn.kitti_batch(0, 2, 1024, 4)
    pts, labels = torch.from_numpy(pts_np).to(dev), torch.from_numpy(lab_np).to(dev)
    net.eval()
    torch.manual_seed(1)
    before = net(pts).detach().clone()
    bucket = FlatGradBucket(net, direct=True)
    try:
        opt = optim.SGD(net.parameters(), lr=0.01, momentum=0.9, bucket=bucket)
        assert opt._flat[0]["g"] is bucket.flat
        torch.manual_seed(1)
        assert torch.equal(net(pts), before)
        net.train()
        losses = []
        for _ in range(4):
            opt.zero_grad()
            torch.manual_seed(1)
            loss = nll_loss(net(pts).reshape(-1, 13), labels.reshape(-1))
            loss.backward()
            assert float(bucket.flat.abs().sum()) > 0
            for p in net.parameters():
                assert p.grad.data_ptr() >= bucket.flat.data_ptr()
            opt.step()
            losses.append(float(loss.detach()))
        assert losses[-1] < losses[0], losses
        next(net.parameters()).grad = None
        with pytest.raises(_lib.Pn2Error):
            opt.step()                                          # a .grad that no longer aliases the flat buffer
    finally:
        pointnet_util.set_direct_grad_accumulation(False)


# ----------------------------------------------------------------------------------------------- 8. two groups
def test_sgd_two_parameter_groups(dev):
    """Per-group lr and momentum, one of them 0 (no buffer for that group): one launch per group."""
    torch.manual_seed(21)
    sizes = [(50, 7), (50,), (9, 3, 1)]
    init = [torch.randn(s) for s in sizes]
    a = [torch.nn.Parameter(t.clone()) for t in init]
    b = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    spec = lambda ps: [{"params": ps[:2], "lr": 1e-2, "momentum": 0.9, "weight_decay": 1e-4},
                       {"params": ps[2:], "lr": 5e-2, "momentum": 0}]
    ref = torch.optim.SGD(spec(a), lr=1e-3, momentum=0.5)
    mine = optim.SGD(spec(b), lr=1e-3, momentum=0.5)
    assert len(mine.param_groups) == 2 and mine._flat[0]["buf"] is not None and mine._flat[1]["buf"] is None
    for t in range(1, 6):
        mine.zero_grad()
        feed(a, b, draw(sizes))
        ref.step()
        mine.step()
        same_bits(flat(b), flat(a), "parameters, step %d" % t)
    same_bits(flat(buffers(mine, b[:2])), flat(buffers(ref, a[:2])), "momentum buffers of group 0")
    assert mine.steps_taken() == [5, 5] and sorted(mine.state_dict()["state"]) == [0, 1]
    with pytest.raises(ValueError):
        optim.SGD(spec(b), lr=1e-3, bucket=object())            # a shared bucket needs a single group
