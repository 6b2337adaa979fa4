"""GPU: PointNet v1 on the HIP library (pointnet12_amd/pointnet.py; csrc/pointnet_v1.hip).

Kernel level against fp64 on fixed operands (the per-cloud transform and its gradients, max of BatchNorm output without a ReLU and its
backward, the factorised broadcast-concat layer's forward and column sums), module level against the reference's recorded step
(tests/golden/g13_pointnet.npz, the bounds of tests/test_pointnet_v1_cpu.py), one S3DIS-shape training step against the fp64
restatement (each tensor within 4x the distance of a stock-torch fp32 run of the same restatement), eval on one 25 000-point cloud,
and a dispatch-mode census: no ATen GEMM, convolution, BatchNorm or max-reduction on per-point rows."""
import pytest
import torch
import torch.nn as nn

from conftest import golden
import pointnet_v1_ref as V
from test_pointnet_v1_cpu import bias_before_bn, compare_step, run_restatement

pytestmark = pytest.mark.gpu


def _lib():
    from pointnet12_amd import _lib as L
    return L


def _rows_of(t, k):
    """[P, k] -> [P, round4(k)] zero padded, fp32 contiguous."""
    kp = (k + 3) & ~3
    out = torch.zeros(t.shape[0], kp, device=t.device, dtype=torch.float32)
    out[:, :k] = t
    return out


@pytest.mark.parametrize("k", [3, 4, 9, 64, 128])
def test_point_transform_against_fp64(dev, k):
    L = _lib()
    lib = L.load()
    st = L.stream()
    gen = torch.Generator(device="cpu").manual_seed(100 + k)
    for B, N in ((1, 500), (16, 500), (1, 4096), (16, 4096), (1, 25000), (16, 25000)):
        if k == 128 and B == 16 and N == 25000:
            N = 12500                              # (keeps the fp64 operands of this case under 1 GB)
        X = torch.randn(B * N, k, generator=gen).to(dev)
        T = (torch.randn(B, k, k, generator=gen) / k ** 0.5).to(dev)
        D = torch.randn(B * N, k, generator=gen).to(dev)
        Xr, Dr = _rows_of(X, k), _rows_of(D, k)
        kp = Xr.shape[1]
        out = torch.full((B * N, kp), float("nan"), device=dev)
        L.check(lib.pn2_point_transform(Xr.data_ptr(), kp, T.data_ptr(), B, N, k, out.data_ptr(), kp, st), "pn2_point_transform")
        ref = torch.bmm(X.double().view(B, N, k), T.double()).view(B * N, k)
        assert float((out[:, :k].double() - ref).abs().max()) <= 3e-6 * float(ref.abs().max()), (B, N, k)
        assert bool((out[:, k:] == 0).all())
        ws = torch.empty(int(lib.pn2_point_transform_workspace_bytes(B, N, k)), device=dev, dtype=torch.uint8)
        dX = torch.full((B * N, kp), float("nan"), device=dev)
        dT = torch.empty(B, k, k, device=dev)
        dT2 = torch.empty(B, k, k, device=dev)
        for target in (dT, dT2):
            L.check(lib.pn2_point_transform_bwd(Dr.data_ptr(), kp, Xr.data_ptr(), kp, T.data_ptr(), B, N, k, dX.data_ptr(), kp,
                                                target.data_ptr(), ws.data_ptr(), st), "pn2_point_transform_bwd")
        ref_dx = torch.bmm(D.double().view(B, N, k), T.double().transpose(1, 2)).view(B * N, k)
        ref_dt = torch.bmm(X.double().view(B, N, k).transpose(1, 2), D.double().view(B, N, k))
        assert float((dX[:, :k].double() - ref_dx).abs().max()) <= 3e-6 * float(ref_dx.abs().max()), (B, N, k)
        assert bool((dX[:, k:] == 0).all())
        assert float((dT.double() - ref_dt).abs().max()) <= 1e-5 * float(ref_dt.abs().max()), (B, N, k)
        assert torch.equal(dT, dT2), "dT differs between two launches"
        del X, D, Xr, Dr, out, dX, dT, dT2, ref, ref_dx, ref_dt, ws


def _affine(mean, gamma, beta, var, eps=1e-5):
    C = mean.shape[0]
    ld = (C + 3) & ~3
    invstd = 1.0 / torch.sqrt(var.double() + eps)
    a = torch.zeros(4 * ld, dtype=torch.float32, device=mean.device)
    a[:C] = mean
    a[ld:ld + C] = (gamma.double() * invstd).float()
    a[2 * ld:2 * ld + C] = beta
    a[3 * ld:3 * ld + C] = invstd.float()
    return a


def test_bn_max_and_its_backward(dev):
    L = _lib()
    lib = L.load()
    st = L.stream()
    gen = torch.Generator(device="cpu").manual_seed(7)
    for G, K, C in ((4, 500, 64), (2, 4095, 1024), (1, 25000, 96), (16, 4096, 1024)):
        Y = torch.randn(G * K, C, generator=gen).to(dev)
        gamma = torch.rand(C, generator=gen).to(dev) + 0.5
        gamma[1::3] *= -1.0                                  # gamma < 0: the smallest y wins
        gamma[2::7] = 0.0                                    # gamma == 0: every row gives beta -> row 0
        beta = torch.randn(C, generator=gen).to(dev)
        mean = torch.randn(C, generator=gen).to(dev) * 0.1
        var = torch.rand(C, generator=gen).to(dev) + 0.5
        aff = _affine(mean, gamma, beta, var)
        ld = (C + 3) & ~3
        out = torch.empty(G, ld, device=dev)
        arg = torch.empty(G, ld, device=dev, dtype=torch.int32)
        L.check(lib.pn2_bn_max(Y.data_ptr(), C, aff.data_ptr(), G, K, C, out.data_ptr(), ld, arg.data_ptr(), st), "pn2_bn_max")
        sc = aff[ld:ld + C]
        bnv = ((Y - mean).double() * sc.double() + beta.double()).float().view(G, K, C)      # fma(y - mean, scale, beta)
        want = bnv.max(dim=1).values
        assert torch.equal(out[:, :C], want)
        # the first row attaining the maximum
        first = (bnv == want[:, None, :]).int().argmax(dim=1)
        assert torch.equal(arg[:, :C].long(), first)
        zero = (gamma == 0)
        assert bool((arg[:, :C][:, zero] == 0).all())
        ypos = Y.view(G, K, C)
        neg = gamma < 0
        assert torch.equal(ypos.gather(1, arg[:, None, :C].long())[:, 0, neg], ypos.min(dim=1).values[:, neg])
        # backward
        dOut = torch.randn(G, C, generator=gen).to(dev)
        dzp = torch.full((G, ld), float("nan"), device=dev)
        red = torch.zeros(8 * 2 * C, device=dev, dtype=torch.float64)
        L.check(lib.pn2_pool_bwd_reduce_noact(dOut.data_ptr(), C, arg.data_ptr(), ld, Y.data_ptr(), C, aff.data_ptr(), G, K, C,
                                              dzp.data_ptr(), red.data_ptr(), st), "pn2_pool_bwd_reduce_noact")
        assert torch.equal(dzp[:, :C], dOut)
        ysel = ypos.gather(1, arg[:, None, :C].long())[:, 0, :].double()
        yhat = (ysel - mean.double()) / torch.sqrt(var.double() + 1e-5)
        r = red.view(8, 2, C).sum(0)
        want0 = dOut.double().sum(0)
        want1 = (dOut.double() * yhat).sum(0)
        assert float((r[0] - want0).abs().max()) <= 1e-5 * max(1.0, float(want0.abs().max()))
        assert float((r[1] - want1).abs().max()) <= 1e-5 * max(1.0, float(want1.abs().max()))


def test_gbias_forward_and_group_colsum(dev):
    L = _lib()
    lib = L.load()
    st = L.stream()
    gen = torch.Generator(device="cpu").manual_seed(9)
    for B, N in ((2, 500), (16, 4096)):
        P, K, C, CG = B * N, 64, 512, 1024
        X = torch.randn(P, K, generator=gen).to(dev)
        W = (torch.randn(C, CG + K, generator=gen) / 30).to(dev)
        b = torch.randn(C, generator=gen).to(dev)
        g = torch.randn(B, CG, generator=gen).to(dev)
        gterm = (g.double() @ W[:, :CG].double().T).float().contiguous()
        Y = torch.empty(P, C, device=dev)
        stats = torch.zeros(8 * 2 * C, device=dev, dtype=torch.float64)
        L.check(lib.pn2_conv1x1_fwd_gbias(X.data_ptr(), K, W.data_ptr() + 4 * CG, CG + K, b.data_ptr(), gterm.data_ptr(), C, N, Y.data_ptr(),
                                          C, P, K, C, stats.data_ptr(), st), "pn2_conv1x1_fwd_gbias")
        ref = X.double() @ W[:, CG:].double().T + b.double() + gterm.double().repeat_interleave(N, 0)
        assert float((Y.double() - ref).abs().max()) <= 3e-6 * float(ref.abs().max())
        s = stats.view(8, 2, C).sum(0)
        Yd = Y.double()
        assert float((s[0] - Yd.sum(0)).abs().max()) <= 1e-9 * float(Yd.abs().sum(0).max())
        assert float((s[1] - (Yd * Yd).sum(0)).abs().max()) <= 1e-9 * float((Yd * Yd).sum(0).max())
        # column sums of dY = c0 dZ + q1 (y - mean) + q0 per cloud
        dZ = torch.randn(P, C, generator=gen).to(dev)
        coef = torch.zeros(4 * C, device=dev)
        coef[:C] = torch.rand(C, generator=gen).to(dev) + 0.5
        coef[C:2 * C] = torch.randn(C, generator=gen).to(dev) * 1e-3
        coef[2 * C:3 * C] = torch.randn(C, generator=gen).to(dev) * 1e-3
        coef[3 * C:] = Y.mean(0)
        out = torch.full((B, C), float("nan"), device=dev)
        ws = torch.empty(int(lib.pn2_group_colsum_workspace_bytes(P, N, C)), device=dev, dtype=torch.uint8)
        L.check(lib.pn2_group_colsum(dZ.data_ptr(), C, Y.data_ptr(), C, coef.data_ptr(), P, N, C, out.data_ptr(), C, ws.data_ptr(), st),
                "pn2_group_colsum")
        c = coef.double().view(4, C)
        dY = c[0] * dZ.double() + c[1] * (Y.double() - c[3]) + c[2]
        want = dY.view(B, N, C).sum(1)
        assert float((out.double() - want).abs().max()) <= 1e-5 * float(dY.abs().view(B, N, C).sum(1).max())
        out2 = torch.empty_like(out)
        L.check(lib.pn2_group_colsum(dZ.data_ptr(), C, Y.data_ptr(), C, coef.data_ptr(), P, N, C, out2.data_ptr(), C, ws.data_ptr(), st),
                "pn2_group_colsum")
        assert torch.equal(out, out2)


def _library_step(tag, g, dev):
    """The recorded training step on the library: returns (net, x, lp, trans, trans_feat, loss, lp_eval, tf_eval)."""
    from pointnet12_amd import pointnet as M
    torch.manual_seed(0)
    net = M.PointNetSeg(13, 9, True) if tag == "seg" else M.PointNetCls(40, True)
    net.to(dev).train()
    for m in net.modules():
        if isinstance(m, nn.Dropout):
            m.eval()
    seen = []
    orig = M._stn_from_rows

    def spy(stn, rows, B, N, k):
        t = orig(stn, rows, B, N, k)
        seen.append(t)
        return t
    M._stn_from_rows = spy
    try:
        x = torch.from_numpy(g[tag + "/x"]).to(dev).requires_grad_(True)
        lp, tf = net(x)
    finally:
        M._stn_from_rows = orig
    labels = torch.from_numpy(g[tag + "/labels"]).to(dev)
    C = lp.shape[-1]
    loss = torch.nn.functional.nll_loss(lp.reshape(-1, C), labels.reshape(-1)) + 0.001 * M.feature_transform_reguliarzer(tf)
    loss.backward()
    net.eval()
    with torch.no_grad():
        lp_e, tf_e = net(x.detach())
    return net, x, lp, seen[0], tf, loss, lp_e, tf_e


class _Grads:
    """V.Params-like view of a module's gradients and running statistics (for compare_step)."""

    def __init__(self, net):
        self.net = net
        self.state = {k: v for k, v in net.state_dict().items() if k.endswith(("running_mean", "running_var"))}

    def grads(self):
        return {k: p.grad for k, p in self.net.named_parameters()}


@pytest.mark.parametrize("tag", ["seg", "cls"])
def test_networks_against_the_reference_step(dev, tag):
    g = golden("g13_pointnet.npz")
    net, x, lp, trans, tf, loss, lp_e, tf_e = _library_step(tag, g, dev)
    errs = compare_step(tag, g, _Grads(net), x.grad, lp, trans, tf, loss, lp_e, tf_e)
    # the stock PyTorch parts of the network (the [B, .] heads) run in fp32 on this GPU: a tensor may also sit within 4x of where a
    # stock-torch fp32 run of the restatement on the same GPU lands against the same record
    P, xf, lpf, transf, tff, lossf, lpef, tfef = run_restatement(tag, g, torch.float32, dev)
    f32 = {e[1]: e[2] for e in compare_step(tag, g, P, xf.grad, lpf, transf, tff, lossf, lpef, tfef)}
    bad = sorted([e for e in errs if e[2] > max(e[3], 4.0 * f32[e[1]])], reverse=True)
    assert not bad, "%s: %d tensors outside the bound, worst %s" % (tag, len(bad), bad[:5])


def _restated_step(sd, x, labels, dtype, dev, formulation="factorised", pick=None):
    P = V.Params(sd, dtype, dev)
    xx = x.to(dtype).detach().requires_grad_(True)
    lp, trans, tf = V.seg_forward(P, xx, True, True, formulation, pick)
    loss = V.train_loss(lp, labels, tf)
    loss.backward()
    out = {"log_probs": lp.detach(), "trans_feat": tf.detach(), "loss": loss.detach().reshape(1), "grad/x": xx.grad}
    out.update({"grad/" + k: v for k, v in P.grads().items()})
    return out


def test_s3dis_shape_training_step_against_fp64(dev):
    """B = 16 x 4096 x 9, PointNetSeg(13, 9, True): every tensor within 4x the distance of stock-torch fp32 to fp64."""
    from pointnet12_amd import pointnet as M
    torch.manual_seed(0)
    net = M.PointNetSeg(13, 9, True).to(dev).train()
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    gen = torch.Generator(device="cpu").manual_seed(21)
    B, N = 16, 4096
    x = torch.randn(B, 9, N, generator=gen).to(dev)
    labels = torch.randint(0, 13, (B, N), generator=gen).to(dev)
    # the library's arg-max rows of the three max-pools over the points (STN, feature STN, encoder): at 16 x 1024 channels over
    # 4096 points some maxima tie to within fp32 rounding, and the gradient of a max follows whichever row it picked -- both
    # restatements are evaluated at the library's choice (any of the tied rows is a correct answer)
    picks = {}
    orig_mlp, orig_max = M.shared_mlp, M.conv_bn_max

    def spy_mlp(rows, c_in, convs, bns, pool, training, dest=None):
        out = orig_mlp(rows, c_in, convs, bns, pool, training, dest)
        if pool:                                  # (the STN's pooled stack runs first, then the feature STN's)
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
        lp, tf = net(xx)
    finally:
        M.shared_mlp, M.conv_bn_max = orig_mlp, orig_max
    assert sorted(picks) == ["feat.", "feat.fstn.", "feat.stn."]
    ref = _restated_step(sd, x, labels, torch.float64, dev, pick=picks)
    f32 = _restated_step(sd, x, labels, torch.float32, dev, pick=picks)
    loss = torch.nn.functional.nll_loss(lp.reshape(-1, 13), labels.reshape(-1)) + 0.001 * M.feature_transform_reguliarzer(tf)
    loss.backward()
    lib = {"log_probs": lp.detach(), "trans_feat": tf.detach(), "loss": loss.detach().reshape(1), "grad/x": xx.grad}
    lib.update({"grad/" + k: p.grad for k, p in net.named_parameters()})
    bad = []
    for k, r in ref.items():
        d_lib = float((lib[k].double() - r).abs().max())
        d_f32 = float((f32[k].double() - r).abs().max())
        scale = float(r.abs().max())
        if bias_before_bn(k):
            scale = float(ref[k[:-len("bias")] + "weight"].abs().max())
        if d_lib > max(4.0 * d_f32, 1e-6 * scale):
            bad.append((k, d_lib, d_f32, scale))
    assert not bad, "%d tensors beyond 4x the fp32 distance: %s" % (len(bad), bad[:6])


def test_eval_on_one_25000_point_cloud(dev):
    """PointNetSeg(19, 4, True).eval() under no_grad on one 25 000-point cloud (the viewer's shape) against fp64."""
    from pointnet12_amd import pointnet as M
    torch.manual_seed(0)
    net = M.PointNetSeg(19, 4, True)
    gen = torch.Generator(device="cpu").manual_seed(5)
    with torch.no_grad():
        for name, buf in net.named_buffers():
            if name.endswith("running_mean"):
                buf.copy_(torch.randn(buf.shape, generator=gen) * 0.1)
            elif name.endswith("running_var"):
                buf.copy_(torch.rand(buf.shape, generator=gen) + 0.5)
    net.to(dev).eval()
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    x = torch.randn(1, 4, 25000, generator=gen).to(dev)
    with torch.no_grad():
        lp, tf = net(x)
        outs = []
        for dt in (torch.float64, torch.float32):
            P = V.Params(sd, dt, dev)
            outs.append(V.seg_forward(P, x.to(dt), False, True))
    (r_lp, _, r_tf), (f_lp, _, f_tf) = outs
    assert lp.shape == (1, 25000, 19) and tf.shape == (1, 64, 64)
    for got, ref, f in ((lp, r_lp, f_lp), (tf, r_tf, f_tf)):
        d = float((got.double() - ref).abs().max())
        assert d <= max(4.0 * float((f.double() - ref).abs().max()), 1e-5 * float(ref.abs().max())), d


GEMM_LIKE = ("mm", "addmm", "bmm", "baddbmm", "matmul", "convolution", "conv1d", "cudnn_convolution", "miopen_convolution",
             "native_batch_norm", "batch_norm", "_native_batch_norm_legit", "cudnn_batch_norm", "miopen_batch_norm", "max", "amax",
             "max_pool", "linear", "einsum")


def test_no_aten_gemm_on_per_point_rows(dev):
    from torch.utils._python_dispatch import TorchDispatchMode
    from pointnet12_amd import pointnet as M
    B, N = 4, 3000

    class Census(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.bad = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            name = func.overloadpacket.__name__
            if name.lstrip("_").startswith(GEMM_LIKE) and name != "maximum":
                for a in list(args) + list((kwargs or {}).values()):
                    if torch.is_tensor(a) and any(d in (N, B * N) for d in a.shape):
                        self.bad.append((name, tuple(a.shape)))
            return func(*args, **(kwargs or {}))

    torch.manual_seed(0)
    net = M.PointNetSeg(13, 9, True).to(dev).train()
    x = torch.randn(B, 9, N, device=dev, requires_grad=True)
    labels = torch.randint(0, 13, (B, N), device=dev)
    census = Census()
    with census:
        lp, tf = net(x)
        loss = torch.nn.functional.nll_loss(lp.reshape(-1, 13), labels.reshape(-1)) + 0.001 * M.feature_transform_reguliarzer(tf)
        loss.backward()
    assert not census.bad, census.bad[:10]
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())
