"""CPU: the PointNetDenseCls / PointNetLoss drop-in contract (pointnet12_amd/pointnet.py against the reference's model/pointnet.py,
recorded in tests/golden/g14_densecls.npz by tools/make_golden_densecls.py): seeded state_dicts, the fp64 restatement
(tests/densecls_ref.py) against the reference's recorded training step in both formulations, PointNetLoss, and the argument checks
of the ABI 13 entry points (no GPU needed).  The bound of every tensor is max(1e-5 x its largest |entry|, 3 x the reference's own
8-thread vs 1-thread movement of that tensor), as for g13."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden
from test_oracle_golden import state_sha256
import densecls_ref as D
import pointnet_v1_ref as V

SLICE_ROWS = 1


def bias_before_bn(key):
    """Biases of conv / fc layers that feed a BatchNorm: their gradient is zero up to rounding (compared on the weight's scale)."""
    parts = key.split(".")
    return parts[-1] == "bias" and parts[-2].startswith(("conv", "fc")) and parts[-2] not in ("fc3", "convs4")


def scale_of(g, key):
    k = "step/" + key
    return float(g[k + "/absmax"]) if k + "/absmax" in g else float(np.abs(g[k]).max())


def check(g, key, got, errs, scale=None):
    """got: the full tensor; the fixture may hold only its first SLICE_ROWS rows."""
    ref = np.asarray(g["step/" + key], np.float64)
    got = np.asarray(got.detach().cpu().double().numpy() if torch.is_tensor(got) else got, np.float64)
    if "step/" + key + "/absmax" in g:
        got = got[:SLICE_ROWS]
    assert got.shape == ref.shape, "%s: shape %s vs %s" % (key, got.shape, ref.shape)
    if scale is None:
        scale = scale_of(g, key)
    bound = max(1e-5 * scale, 3.0 * float(g["step/noise/" + key]))
    err = float(np.abs(got - ref).max())
    errs.append((err / bound, key, err, bound))


def inputs(g, dtype=torch.float64, device="cpu"):
    x = torch.from_numpy(g["step/x"]).to(device=device, dtype=dtype)
    cls = torch.from_numpy(g["step/cls"]).to(device)
    seg = torch.from_numpy(g["step/seg"]).to(device)
    onehot = torch.eye(16, dtype=dtype, device=device)[cls]
    return x, cls, seg, onehot


def run_restatement(g, dtype=torch.float64, device="cpu", formulation="factorised"):
    """The recorded step on the restatement: (P, x, outputs dict, eval outputs)."""
    from pointnet12_amd import pointnet as M
    torch.manual_seed(0)
    P = V.Params(M.PointNetDenseCls().state_dict(), dtype, device)
    x, cls, seg, onehot = inputs(g, dtype, device)
    x.requires_grad_(True)
    net, net2, trans, tf = D.dense_forward(P, x, onehot, True, formulation)
    loss, seg_loss, label_loss = D.dense_loss(net, cls, net2, seg, tf, weight=0.5)
    loss1 = D.dense_loss(net, cls, net2, seg, tf)
    loss.backward()
    with torch.no_grad():
        ne, n2e, _, tfe = D.dense_forward(P, x.detach(), onehot, False, formulation)
    out = {"net": net, "net2": net2, "trans": trans, "trans_feat": tf, "loss": loss, "seg_loss": seg_loss, "label_loss": label_loss,
           "loss1/loss": loss1[0], "loss1/seg_loss": loss1[1], "loss1/label_loss": loss1[2]}
    return P, x, out, {"eval/net": ne, "eval/net2": n2e, "eval/trans_feat": tfe}


def compare_step(g, grads, state, x_grad, out, ev):
    errs = []
    for k, v in out.items():
        check(g, k, float(v.detach()) if v.dim() == 0 else v, errs)
    check(g, "grad/x", x_grad, errs)
    for k, v in grads.items():
        sc = scale_of(g, "grad/" + k[:-len("bias")] + "weight") if bias_before_bn(k) else None
        check(g, "grad/" + k, v, errs, sc)
    for k, v in state.items():
        if k.endswith(("running_mean", "running_var")):
            check(g, "after/" + k, v, errs)
    for k, v in ev.items():
        check(g, k, v, errs)
    return errs


def test_state_dicts_match_the_reference():
    from pointnet12_amd import pointnet as M
    g = golden("g14_densecls.npz")
    for tag in ("PointNetDenseCls", "PointNetDenseCls_5_7"):
        torch.manual_seed(0)
        net = M.PointNetDenseCls(*[int(a) for a in g[tag + "/args"]])
        sd = net.state_dict()
        assert list(sd) == [str(k) for k in g[tag + "/keys"]], "%s: state_dict keys / order differ" % tag
        assert ["x".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g[tag + "/shapes"]], "%s: shapes differ" % tag
        assert [str(v.dtype) for v in sd.values()] == [str(d) for d in g[tag + "/dtypes"]], "%s: dtypes differ" % tag
        assert state_sha256(net) == str(g[tag + "/sha256"]), "%s: seeded initial values differ" % tag


def test_reference_checkpoint_keys_load():
    """partseg.py saves the state_dict of nn.DataParallel(model): every key carries ``module.``."""
    from pointnet12_amd import pointnet as M
    from pointnet12_amd.pointnet2 import load_reference_state
    torch.manual_seed(1)
    src = M.PointNetDenseCls()
    ckpt = {"module." + k: v.clone() for k, v in src.state_dict().items()}
    dst = M.PointNetDenseCls()
    load_reference_state(dst, ckpt)
    for k, v in dst.state_dict().items():
        assert torch.equal(v, src.state_dict()[k]), k


def test_restatement_reproduces_the_reference_training_step():
    """Within the record's bound, or within 2x where an fp32 evaluation of the same restatement lands (the record is fp32 too:
    fstn.fc3.bias, behind the 4944-deep convs1 and the 128 x 128 feature transform, moves 3e-5 x its scale between fp32 and fp64)."""
    g = golden("g14_densecls.npz")
    P, x, out, ev = run_restatement(g)
    errs = compare_step(g, P.grads(), P.state, x.grad, out, ev)
    P32, x32, out32, ev32 = run_restatement(g, torch.float32)
    f32 = {e[1]: e[2] for e in compare_step(g, P32.grads(), P32.state, x32.grad, out32, ev32)}
    bad = sorted(e for e in errs if e[2] > max(e[3], 2.0 * f32[e[1]]))
    assert not bad, "%d tensors outside the bound, worst %s" % (len(bad), bad[-3:])


def test_concat_formulation_equals_the_factorised_one():
    g = golden("g14_densecls.npz")
    a = run_restatement(g)
    b = run_restatement(g, formulation="concat")
    for k in ("net", "net2", "loss"):
        assert float((a[2][k] - b[2][k]).abs().max()) < 1e-12, k
    assert float((a[1].grad - b[1].grad).abs().max()) < 1e-12
    ga, gb = a[0].grads(), b[0].grads()
    for k in ga:
        assert float((ga[k] - gb[k]).abs().max()) < 1e-12 * max(1.0, float(ga[k].abs().max())), k


def test_pointnet_loss_matches_the_reference_for_both_weights():
    from pointnet12_amd import pointnet as M
    g = golden("g14_densecls.npz")
    _, cls, seg, _ = inputs(g)
    torch.manual_seed(3)
    net = torch.randn(8, 16, dtype=torch.float64)                 # raw logits: nll_loss takes them as they are
    net2 = torch.log_softmax(torch.randn(8, 500, 50, dtype=torch.float64), -1)
    tf = torch.eye(128, dtype=torch.float64)[None] + 0.01 * torch.randn(8, 128, 128, dtype=torch.float64)
    flat, target = net2.reshape(-1, 50), seg.reshape(-1)
    for w in (1, 0.5):
        loss, seg_loss, label_loss = M.PointNetLoss(weight=w)(net, cls, flat, target, tf)
        want = D.dense_loss(net, cls, net2, seg, tf, weight=w)
        assert abs(float(loss) - float(want[0])) < 1e-12 and abs(float(seg_loss) - float(want[1])) < 1e-12
        assert abs(float(label_loss) - float(-net[torch.arange(8), cls].mean())) < 1e-12
    assert M.PointNetLoss().weight == 1 and M.PointNetLoss().mat_diff_loss_scale == 0.001
    # the recorded losses of the reference (weight 0.5 and the default 1) on the restatement's outputs
    _, _, out, _ = run_restatement(g)
    for k in ("loss", "seg_loss", "label_loss", "loss1/loss", "loss1/seg_loss", "loss1/label_loss"):
        assert abs(float(out[k]) - float(g["step/" + k])) <= max(1e-6, 3.0 * float(g["step/noise/" + k])), k


def test_exports():
    import pointnet12_amd.pointnet as M
    assert {"PointNetDenseCls", "PointNetLoss", "PointNetSeg"} <= set(dir(M))


def test_abi13_argument_checks_need_no_gpu():
    from pointnet12_amd import _lib
    lib = _lib.load()
    EINVAL = -1
    fake = 1 << 20                                              # never dereferenced: every call below fails its host checks
    good = [(fake, 64, 64, None, 0), (fake, 128, 128, None, 0), (fake, 2048, 2048, fake, 0)]

    def fwd(table, n=None, P=4096, W=fake, ldw=4944):
        t = _lib.src_table(table)
        return lib.pn2_conv1x1_fwd_multi(t, len(table) if n is None else n, W, ldw, fake, None, 0, 1, fake, 256, P, 256, None, None)

    def wgrad(table, n=None, P=4096):
        t = _lib.src_table(table)
        return lib.pn2_conv1x1_wgrad_multi(fake, 256, fake, 256, fake, t, len(table) if n is None else n, fake, 4944, None, P, 256, None)

    for call in (fwd, wgrad):
        assert call(good, n=0) == EINVAL                                           # nsrc out of range
        assert call(good * 3, n=9) == EINVAL
        assert call([(fake, 64, 62, None, 0)]) == EINVAL                           # K % 4
        assert call([(fake, 60, 64, None, 0)]) == EINVAL                           # ldx < K
        assert call([(fake, 66, 64, None, 0)]) == EINVAL                           # ldx % 4
        assert call([(None, 64, 64, None, 0)]) == EINVAL                           # NULL source
        assert call([(fake, 64, 64, None, 1)]) == EINVAL                           # ReLU without an affine block
        assert call(good, P=1 << 31) == EINVAL                                     # P >= 2^31
    assert lib.pn2_conv1x1_fwd_multi(None, 1, fake, 4944, fake, None, 0, 1, fake, 256, 10, 256, None, None) == EINVAL
    assert fwd(good, W=None) == EINVAL
    assert fwd(good, ldw=2000) == EINVAL                                           # ldw < sum K
    t = _lib.src_table(good)
    assert lib.pn2_conv1x1_fwd_multi(t, 3, fake, 4944, fake, fake, 250, 4096, fake, 256, 4096, 256, None, None) == EINVAL   # ldg % 4
    assert lib.pn2_conv1x1_fwd_multi(t, 3, fake, 4944, fake, fake, 256, 1000, fake, 256, 4096, 256, None, None) == EINVAL   # P % rpg
    assert lib.pn2_conv1x1_wgrad_multi(None, 256, fake, 256, fake, t, 3, fake, 4944, None, 10, 256, None) == EINVAL
    dx = (ctypes.c_void_p * 2)(fake, fake)
    ld = (ctypes.c_int * 2)(64, 128)
    ks = (ctypes.c_int * 2)(64, 128)
    bad_k = (ctypes.c_int * 2)(64, 126)
    assert lib.pn2_conv1x1_dgrad_multi(fake, 256, fake, 256, fake, fake, 4944, dx, ld, bad_k, 2, 4096, 256, None) == EINVAL
    assert lib.pn2_conv1x1_dgrad_multi(fake, 256, fake, 256, fake, fake, 4944, dx, ld, ks, 0, 4096, 256, None) == EINVAL
    assert lib.pn2_conv1x1_dgrad_multi(fake, 256, fake, 256, fake, fake, 100, dx, ld, ks, 2, 4096, 256, None) == EINVAL
    assert lib.pn2_conv1x1_dgrad_multi(fake, 256, fake, 256, fake, fake, 4944, dx, ld, ks, 2, 1 << 31, 256, None) == EINVAL
    assert lib.pn2_conv1x1_dgrad_multi(fake, 256, fake, 256, fake, None, 4944, dx, ld, ks, 2, 4096, 256, None) == EINVAL
    assert lib.pn2_bn_bwd_reduce_noact_dense(None, 2048, fake, 2048, fake, 2048, fake, 2048, fake, 16, 2048, 2048, fake, 2048, fake,
                                             None) == EINVAL
    assert lib.pn2_bn_bwd_reduce_noact_dense(fake, 2046, fake, 2048, fake, 2048, fake, 2048, fake, 16, 2048, 2048, fake, 2048, fake,
                                             None) == EINVAL
    assert lib.pn2_bn_bwd_reduce_noact_dense(fake, 2048, fake, 2048, fake, 2048, fake, 2048, fake, 1 << 20, 4096, 2048, fake, 2048,
                                             fake, None) == EINVAL


def test_forward_refuses_labels_that_do_not_fit_convs1():
    """convs1 takes 4944 = 2048 + 16 + 2880 channels: the reference's forward fails for any other cat_num, and so does this one."""
    from pointnet12_amd import pointnet as M
    net = M.PointNetDenseCls(5, 7)
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 3, 8), torch.zeros(1, 5))
