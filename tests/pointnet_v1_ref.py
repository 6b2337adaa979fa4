"""fp64 restatement of the PointNet v1 networks (STN3d, STNkd, PointNetEncoder, PointNetCls, PointNetSeg) and the feature-transform
regulariser, written from the published architecture in this project's own words: a test helper, not a port.

Everything is functional over a parameter dictionary keyed like the networks' ``state_dict`` and works on channel-last rows
[B, N, C] (a 1x1 convolution is a matmul with the weight's [C_out, C_in] view).  ``formulation="factorised"`` evaluates the
segmentation head's first layer as W_p x_p + W_g g_b + b (what the HIP library does); ``"concat"`` builds the [B, N, 1088]
concatenation as the reference does -- with torch.bmm for the transforms -- so the stock-torch timing of tools/bench_pointnet.py
runs the reference formulation.
"""
import torch
import torch.nn.functional as F


class Params:
    """Leaf copies of a state_dict in one dtype / device; BatchNorm running statistics are updated in ``self.state``."""

    def __init__(self, state_dict, dtype=torch.float64, device="cpu"):
        self.p, self.state = {}, {}
        for k, v in state_dict.items():
            if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
                self.state[k] = v.detach().to(device=device, dtype=dtype if v.is_floating_point() else v.dtype).clone()
            else:
                self.p[k] = v.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)

    def __getitem__(self, k):
        return self.p[k]

    def grads(self):
        return {k: v.grad for k, v in self.p.items()}


def _linear(P, name, x):
    w = P[name + ".weight"]
    return x @ w.reshape(w.shape[0], -1).transpose(0, 1) + P[name + ".bias"]


def _norm(P, name, x, train, momentum=0.1, eps=1e-5):
    """BatchNorm over every leading position of x [..., C]; training mode updates the running statistics."""
    flat = x.reshape(-1, x.shape[-1])
    if train:
        mu = flat.mean(0)
        var = ((flat - mu) ** 2).mean(0)
        n = flat.shape[0]
        st = P.state
        with torch.no_grad():
            st[name + ".running_mean"].mul_(1 - momentum).add_(momentum * mu.detach())
            st[name + ".running_var"].mul_(1 - momentum).add_(momentum * var.detach() * n / max(n - 1, 1))
            st[name + ".num_batches_tracked"] += 1
    else:
        mu, var = P.state[name + ".running_mean"], P.state[name + ".running_var"]
    return (x - mu) / torch.sqrt(var + eps) * P[name + ".weight"] + P[name + ".bias"]


def _unit(P, conv, bn, x, train):
    return torch.relu(_norm(P, bn, _linear(P, conv, x), train))


def _max_points(h, pick, site):
    """max over the points of h [B, N, C]; pick (optional) {site: rows [B, C]} evaluates it at given rows instead -- where two points
    tie to within rounding, a caller can hold another evaluation to the SAME choice (the gradient of a max follows its arg-max)."""
    if pick is None or site not in pick:
        return h.amax(dim=1)
    return h.gather(1, pick[site][:, None, :]).squeeze(1)


def stn(P, pre, x, train, k, pick=None):
    """x [B, N, k] -> [B, k, k]: three pointwise units, max over the points, three dense layers, plus the identity."""
    h = _unit(P, pre + "conv1", pre + "bn1", x, train)
    h = _unit(P, pre + "conv2", pre + "bn2", h, train)
    h = _unit(P, pre + "conv3", pre + "bn3", h, train)
    v = _max_points(h, pick, pre)
    v = _unit(P, pre + "fc1", pre + "bn4", v, train)
    v = _unit(P, pre + "fc2", pre + "bn5", v, train)
    v = _linear(P, pre + "fc3", v)
    return v.reshape(-1, k, k) + torch.eye(k, dtype=v.dtype, device=v.device)


def _apply(x, t, formulation):
    return torch.bmm(x, t) if formulation == "concat" else torch.einsum("bni,bij->bnj", x, t)


def encoder(P, pre, x, train, feature_transform, formulation="factorised", pick=None):
    """x [B, N, C] -> (global [B, 1024], pointfeat [B, N, 64], trans, trans_feat)."""
    k = x.shape[-1]
    trans = stn(P, pre + "stn.", x, train, k, pick)
    h = _unit(P, pre + "conv1", pre + "bn1", _apply(x, trans, formulation), train)
    trans_feat = None
    if feature_transform:
        trans_feat = stn(P, pre + "fstn.", h, train, 64, pick)
        h = _apply(h, trans_feat, formulation)
    h2 = _unit(P, pre + "conv2", pre + "bn2", h, train)
    y3 = _norm(P, pre + "bn3", _linear(P, pre + "conv3", h2), train)         # no ReLU before the max
    return _max_points(y3, pick, pre), h, trans, trans_feat


def cls_forward(P, x, train, feature_transform):
    """x [B, 3, N] -> (log_probs [B, k], trans, trans_feat); dropout is the identity (the tests switch it off)."""
    g, _, trans, trans_feat = encoder(P, "feat.", x.transpose(1, 2), train, feature_transform)
    v = _unit(P, "fc1", "bn1", g, train)
    v = _unit(P, "fc2", "bn2", v, train)
    return torch.log_softmax(_linear(P, "fc3", v), dim=1), trans, trans_feat


def seg_forward(P, x, train, feature_transform, formulation="factorised", pick=None):
    """x [B, C, N] -> (log_probs [B, N, k], trans, trans_feat)."""
    g, pf, trans, trans_feat = encoder(P, "feat.", x.transpose(1, 2), train, feature_transform, formulation, pick)
    B, N = pf.shape[0], pf.shape[1]
    w1 = P["conv1.weight"].reshape(P["conv1.weight"].shape[0], -1)
    cg = g.shape[1]
    if formulation == "concat":
        cat = torch.cat([g[:, None, :].expand(B, N, cg), pf], dim=2)
        y1 = cat @ w1.transpose(0, 1) + P["conv1.bias"]
    else:
        y1 = pf @ w1[:, cg:].transpose(0, 1) + (g @ w1[:, :cg].transpose(0, 1))[:, None, :] + P["conv1.bias"]
    h = torch.relu(_norm(P, "bn1", y1, train))
    h = _unit(P, "conv2", "bn2", h, train)
    h = _unit(P, "conv3", "bn3", h, train)
    return torch.log_softmax(_linear(P, "conv4", h), dim=-1), trans, trans_feat


def regulariser(t):
    """mean over clouds of || T (T^T - I) ||_F -- the reference's expression, as written."""
    eye = torch.eye(t.shape[1], dtype=t.dtype, device=t.device)
    m = torch.matmul(t, t.transpose(1, 2) - eye)
    return (m * m).sum(dim=(1, 2)).sqrt().mean()


def train_loss(log_probs, labels, trans_feat, scale=0.001):
    """nll + scale * regulariser, the training loss of the reference drivers."""
    C = log_probs.shape[-1]
    loss = F.nll_loss(log_probs.reshape(-1, C), labels.reshape(-1))
    if trans_feat is not None:
        loss = loss + scale * regulariser(trans_feat)
    return loss
