"""CPU: the PointNet v1 drop-in contract (pointnet12_amd/pointnet.py against the reference's model/pointnet.py, recorded in
tests/golden/g13_pointnet.npz by tools/make_golden_pointnet.py): seeded state_dicts of all six networks, and the fp64 restatement
(tests/pointnet_v1_ref.py) against the reference's recorded training step -- outputs, loss, input and parameter gradients, running
statistics and the eval-mode outputs after the step.  The bound of every tensor is max(1e-5 x its largest |entry|, 3 x the reference's
own 8-thread vs 1-thread movement of that tensor)."""
import numpy as np
import torch

from conftest import golden
from test_oracle_golden import state_sha256
import pointnet_v1_ref as V

NETS = (("STN3d", "STN3d"), ("STNkd", "STNkd"), ("PointNetCls", "PointNetCls"), ("PointNetCls_noft", "PointNetCls"),
        ("PointNetSeg", "PointNetSeg"), ("PointNetSeg_kitti", "PointNetSeg"))
SLICE_ROWS = 2


def bias_before_bn(key):
    """Biases of conv / fc layers that feed a BatchNorm: their gradient is zero up to rounding (compared on the weight's scale)."""
    parts = key.split(".")
    return parts[-1] == "bias" and parts[-2].startswith(("conv", "fc")) and parts[-2] not in ("fc3", "conv4")


def scale_of(g, tag, key):
    k = tag + "/" + key
    return float(g[k + "/absmax"]) if k + "/absmax" in g else float(np.abs(g[k]).max())


def check(g, tag, key, got, errs, scale=None):
    """got: the full tensor (fp64); the fixture may hold only its first SLICE_ROWS rows."""
    ref = np.asarray(g[tag + "/" + key], np.float64)
    got = np.asarray(got.detach().cpu().double().numpy() if torch.is_tensor(got) else got, np.float64)
    if tag + "/" + key + "/absmax" in g:
        got = got[:SLICE_ROWS]
    assert got.shape == ref.shape, "%s/%s: shape %s vs %s" % (tag, key, got.shape, ref.shape)
    if scale is None:
        scale = scale_of(g, tag, key)
    bound = max(1e-5 * scale, 3.0 * float(g[tag + "/noise/" + key]))
    err = float(np.abs(got - ref).max())
    errs.append((err / bound, key, err, bound))


def test_state_dicts_match_the_reference():
    from pointnet12_amd import pointnet as M
    g = golden("g13_pointnet.npz")
    for tag, cls in NETS:
        torch.manual_seed(0)
        net = getattr(M, cls)(*[int(a) for a in g[tag + "/args"]])
        sd = net.state_dict()
        assert list(sd) == [str(k) for k in g[tag + "/keys"]], "%s: state_dict keys / order differ" % tag
        assert ["x".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g[tag + "/shapes"]], "%s: shapes differ" % tag
        assert [str(v.dtype) for v in sd.values()] == [str(d) for d in g[tag + "/dtypes"]], "%s: dtypes differ" % tag
        assert state_sha256(net) == str(g[tag + "/sha256"]), "%s: seeded initial values differ" % tag


def run_restatement(tag, g, dtype=torch.float64, device="cpu", formulation="factorised"):
    """The recorded training step on the fp64 restatement: returns (P, x, lp, trans, trans_feat, loss, lp_eval, tf_eval)."""
    from pointnet12_amd import pointnet as M
    torch.manual_seed(0)
    net = M.PointNetSeg(13, 9, True) if tag == "seg" else M.PointNetCls(40, True)
    P = V.Params(net.state_dict(), dtype, device)
    x = torch.from_numpy(g[tag + "/x"]).to(device=device, dtype=dtype).requires_grad_(True)
    labels = torch.from_numpy(g[tag + "/labels"]).to(device)
    if tag == "seg":
        lp, trans, tf = V.seg_forward(P, x, True, True, formulation)
    else:
        lp, trans, tf = V.cls_forward(P, x, True, True)
    loss = V.train_loss(lp, labels, tf)
    loss.backward()
    with torch.no_grad():
        if tag == "seg":
            lp_e, _, tf_e = V.seg_forward(P, x, False, True, formulation)
        else:
            lp_e, _, tf_e = V.cls_forward(P, x, False, True)
    return P, x, lp, trans, tf, loss, lp_e, tf_e


def compare_step(tag, g, P, x_grad, lp, trans, tf, loss, lp_e, tf_e, running=True):
    errs = []
    check(g, tag, "log_probs", lp, errs)
    check(g, tag, "trans", trans, errs)
    check(g, tag, "trans_feat", tf, errs)
    check(g, tag, "loss", float(loss.detach()), errs)
    check(g, tag, "grad/x", x_grad, errs)
    grads = P.grads()
    for k, v in grads.items():
        sc = scale_of(g, tag, "grad/" + k[:-len("bias")] + "weight") if bias_before_bn(k) else None
        check(g, tag, "grad/" + k, v, errs, sc)
    if running:
        for k, v in P.state.items():
            if k.endswith(("running_mean", "running_var")):
                check(g, tag, "after/" + k, v, errs)
        check(g, tag, "eval/log_probs", lp_e, errs)
        check(g, tag, "eval/trans_feat", tf_e, errs)
    return errs


def test_restatement_reproduces_the_reference_training_step():
    g = golden("g13_pointnet.npz")
    for tag in ("seg", "cls"):
        P, x, lp, trans, tf, loss, lp_e, tf_e = run_restatement(tag, g)
        errs = compare_step(tag, g, P, x.grad, lp, trans, tf, loss, lp_e, tf_e)
        worst = max(errs)
        assert worst[0] <= 1.0, "%s: %s off by %.3g (bound %.3g)" % (tag, worst[1], worst[2], worst[3])


def test_concat_formulation_equals_the_factorised_one():
    g = golden("g13_pointnet.npz")
    a = run_restatement("seg", g)
    b = run_restatement("seg", g, formulation="concat")
    assert float((a[2] - b[2]).abs().max()) < 1e-12
    assert float((a[1].grad - b[1].grad).abs().max()) < 1e-12


def test_regulariser_matches_the_reference():
    from pointnet12_amd import pointnet as M
    g = golden("g13_pointnet.npz")
    for tag in ("seg", "cls"):
        t = torch.from_numpy(g[tag + "/trans_feat"]).double()            # (the recorded clouds)
        want = float(g[tag + "/reg_slice"])
        assert abs(float(M.feature_transform_reguliarzer(t)) - want) <= 1e-6 * max(1.0, abs(want))
        assert abs(float(V.regulariser(t)) - want) <= 1e-6 * max(1.0, abs(want))
        assert M.feature_transform_regularizer is M.feature_transform_reguliarzer
    # and it is T (T^T - I), not T T^T - I
    t = torch.eye(3, dtype=torch.float64)[None] * 2.0
    assert abs(float(M.feature_transform_reguliarzer(t)) - 12.0 ** 0.5) < 1e-12          # T T^T - I: 27 ** 0.5
