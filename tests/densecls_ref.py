"""fp64 restatement of PointNetDenseCls and PointNetLoss (ShapeNet part segmentation), written from the published architecture in this
project's own words: a test helper, not a port.  It reuses the building blocks of tests/pointnet_v1_ref.py (parameter dictionary,
channel-last rows [B, N, C], BatchNorm with running statistics, the STNs).

Two formulations of convs1, the 1x1 conv over the 4944-channel concatenation [cat(out_max, label) * N, out1, out2, out3, out4, out5]:
``"concat"`` builds that concatenation (with torch.bmm for the transforms) as the reference does -- the stock-torch timing of
tools/bench_densecls.py runs it; ``"factorised"`` evaluates W_g g_b once per cloud plus one product per per-point source, what the HIP
library does.  Dropout is the identity (the tests switch it off).
"""
import torch
import torch.nn.functional as F

import pointnet_v1_ref as V

SOURCES = ("out1", "out2", "out3", "out4", "out5")


def dense_forward(P, x, label, train, formulation="factorised", pick=None, record=None):
    """x [B, 3, N], label [B, cat_num] one-hot -> (net [B, cat_num] logits, net2 [B, N, part_num] log-probs, trans, trans_feat).
    pick: {site: rows [B, C]} holds the max-pools ("stn.", "fstn.", "out5") to given arg-max rows; record: dict receiving out1..out5."""
    pts = x.transpose(1, 2)
    B, N = pts.shape[0], pts.shape[1]
    trans = V.stn(P, "stn.", pts, train, 3, pick)
    out1 = V._unit(P, "conv1", "bn1", V._apply(pts, trans, formulation), train)
    out2 = V._unit(P, "conv2", "bn2", out1, train)
    out3 = V._unit(P, "conv3", "bn3", out2, train)
    trans_feat = V.stn(P, "fstn.", out3, train, 128, pick)
    out4 = V._unit(P, "conv4", "bn4", V._apply(out3, trans_feat, formulation), train)
    out5 = V._norm(P, "bn5", V._linear(P, "conv5", out4), train)                    # no ReLU: the max and convs1 both see it
    out_max = V._max_points(out5, pick, "out5")
    net = V._unit(P, "fc1", "bnc1", out_max, train)
    net = V._unit(P, "fc2", "bnc2", net, train)
    net = V._linear(P, "fc3", net)                                                  # raw logits
    g = torch.cat([out_max, label.to(out_max.dtype)], 1)
    w = P["convs1.weight"].reshape(P["convs1.weight"].shape[0], -1)
    cg = g.shape[1]
    per_point = (out1, out2, out3, out4, out5)
    if formulation == "concat":
        cat = torch.cat([g[:, None, :].expand(B, N, cg)] + list(per_point), dim=2)
        y = cat @ w.transpose(0, 1) + P["convs1.bias"]
    else:
        y = (g @ w[:, :cg].transpose(0, 1))[:, None, :] + P["convs1.bias"]
        k = cg
        for t in per_point:
            y = y + t @ w[:, k:k + t.shape[2]].transpose(0, 1)
            k += t.shape[2]
    if record is not None:
        record.update(zip(SOURCES, per_point))
    h = torch.relu(V._norm(P, "bns1", y, train))
    h = V._unit(P, "convs2", "bns2", h, train)
    h = V._unit(P, "convs3", "bns3", h, train)
    return net, torch.log_softmax(V._linear(P, "convs4", h), dim=-1), trans, trans_feat


def dense_loss(net, cls, net2, seg, trans_feat, weight=1.0, scale=0.001):
    """(loss, seg_loss, label_loss): weight * nll(net2) + (1 - weight) * nll(net as given) + scale * regulariser."""
    seg_loss = F.nll_loss(net2.reshape(-1, net2.shape[-1]), seg.reshape(-1))
    label_loss = F.nll_loss(net, cls)
    return weight * seg_loss + (1 - weight) * label_loss + scale * V.regulariser(trans_feat), seg_loss, label_loss
