"""GPU: the four autograd functions at the top of pointnet12_amd/pointnet.py -- point_transform, conv_bn_max, global_concat_conv,
dense_seg_head -- one layer at a time against fp64, at shapes the networks never use.

Each layer is restated with the building blocks of tests/pointnet_v1_ref.py (the restatement of tests/densecls_ref.py from out4
on, for the dense head) and differentiated by torch.autograd in fp64: outputs, every input and parameter gradient and the
BatchNorm running statistics (momentum 0.1, unbiased variance) are compared.  Shapes: B in {1, 3}, N in {5, 70}; channel counts
that are no multiples of 4 wherever the function admits them (conv_bn_max 6 -> 10 and 64 -> 17; global_concat_conv C_out 18;
the dense head on a stand-in with conv widths (8, 12, 12, 16), conv5 out 20, convs1 out 18 and cat_num 3, so that [out_max | label]
has 23 columns and takes the padding branch); point_transform k in {3, 5, 64}.  Modes: training, and eval WITH gradients on
non-trivial running statistics (the training = 0 form of pn2_bn_bwd_coef and the dbias outputs of pn2_conv1x1_wgrad); every subset
of inputs requiring a gradient that the code distinguishes; upstream gradients of four layouts: contiguous, row-broadcast (what
.sum(0) hands back: stride (0, 1)), a column slice of a wider matrix, and a non-unit inner stride.

The max and the ReLU are decisions: the operands' seed of every scenario is chosen on the CPU (``scenario``: the first seed from
the scenario's base) so that in fp64 every post-BN value at a ReLU is further from 0 than MARGIN = 1e-4 of the layer's largest
magnitude and every per-(cloud, channel) maximum leads its runner-up by as much; tests/test_pointnet_v1_kernels_ref_cpu.py asserts
those margins, so no entry is left out here.  The tolerance is the strict rule of tests/test_mlp_gpu.py::_check_shared_mlp for
small cases: a tensor is within 3e-5 of its largest entry, or within 4x of what stock torch fp32 achieves on the same restatement
against the same fp64 answer; no flip slack.
"""
import functools

import pytest
import torch
import torch.nn as nn

import pointnet_v1_ref as V

pytestmark = pytest.mark.gpu

MARGIN = 1e-4
SHAPES = ((1, 70), (3, 5), (3, 70), (1, 5))                 # (B, N)
LAYOUTS = ("contiguous", "broadcast", "slice", "strided")
DENSE_WIDTHS, DENSE_C5, DENSE_CO, DENSE_CAT = (8, 12, 12, 16), 20, 18, 3


def r4(c):
    return (c + 3) & ~3


# ------------------------------------------------------------------------------------------------ upstream gradient layouts

class _Relayout(torch.autograd.Function):
    """Identity whose backward hands the gradient on in another memory layout (same values)."""

    @staticmethod
    def forward(ctx, x, layout):
        ctx.layout = layout
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        R, C = g.shape
        if ctx.layout == "slice":
            wide = torch.full((R, C + 5), 7.0, dtype=g.dtype, device=g.device)
            wide[:, 2:2 + C] = g
            return wide[:, 2:2 + C], None
        if ctx.layout == "strided":
            wide = torch.full((R, 2 * C), 7.0, dtype=g.dtype, device=g.device)
            wide[:, ::2] = g
            return wide[:, ::2], None
        return g.contiguous(), None


def upstream(out, layout, gw):
    """A scalar whose gradient arrives at `out` [R, C] in `layout`: gw [R, C] as it is, or its first row for every row."""
    gw = gw.to(out.dtype)
    if layout == "broadcast":
        return (out.sum(0) * gw[0]).sum()
    return (_Relayout.apply(out, layout) * gw).sum()


# ------------------------------------------------------------------------------------------------ scenarios (CPU, seeded)

def _bn_state(gen, pre, C, sd):
    sd[pre + ".weight"] = torch.rand(C, generator=gen) + 0.5
    sd[pre + ".weight"][1::3] *= -1.0
    sd[pre + ".bias"] = torch.randn(C, generator=gen) * 0.3
    sd[pre + ".running_mean"] = torch.randn(C, generator=gen) * 0.1
    sd[pre + ".running_var"] = torch.rand(C, generator=gen) + 0.5
    sd[pre + ".num_batches_tracked"] = torch.zeros((), dtype=torch.long)


def _conv_state(gen, pre, co, ci, sd):
    sd[pre + ".weight"] = torch.randn(co, ci, 1, generator=gen) / ci ** 0.5
    sd[pre + ".bias"] = torch.randn(co, generator=gen) * 0.1


def _rows(gen, P, C):
    t = torch.zeros(P, r4(C))
    t[:, :C] = torch.randn(P, C, generator=gen)
    return t


def draw(kind, shape, B, N, seed):
    """CPU float32 operands of one scenario: {"in": {name: tensor}, "sd": state dict, "gw": upstream weights}."""
    gen = torch.Generator().manual_seed(seed)
    P, sd = B * N, {}
    if kind == "transform":
        k = shape
        ins = {"rows": _rows(gen, P, k), "trans": torch.randn(B, k, k, generator=gen) / k ** 0.5 + torch.eye(k)}
        outs = [(P, k)]
    elif kind == "conv_bn_max":
        ci, co = shape
        ins = {"x": _rows(gen, P, ci)}
        _conv_state(gen, "conv", co, ci, sd)
        _bn_state(gen, "bn", co, sd)
        outs = [(B, co)]
    elif kind == "concat":
        cp, cg, co = shape
        ins = {"pointfeat": torch.randn(P, cp, generator=gen), "g": torch.randn(B, cg, generator=gen)}
        _conv_state(gen, "conv", co, cg + cp, sd)
        _bn_state(gen, "bn", co, sd)
        outs = [(P, co)]
    else:
        ins = {"out%d" % (i + 1): torch.randn(P, w, generator=gen).abs() for i, w in enumerate(DENSE_WIDTHS)}
        ins["label"] = torch.eye(DENSE_CAT)[torch.randint(0, DENSE_CAT, (B,), generator=gen)]
        _conv_state(gen, "conv5", DENSE_C5, DENSE_WIDTHS[3], sd)
        _bn_state(gen, "bn5", DENSE_C5, sd)
        _conv_state(gen, "convs1", DENSE_CO, DENSE_C5 + DENSE_CAT + sum(DENSE_WIDTHS) + DENSE_C5, sd)
        _bn_state(gen, "bns1", DENSE_CO, sd)
        outs = [(B, DENSE_C5), (P, DENSE_CO)]
    return {"in": ins, "sd": sd, "gw": [torch.randn(*s, generator=gen) for s in outs]}


def _lead(z, margins):
    """z [B, N, C] before a max over N: the lead of every maximum over its runner-up, relative to the largest magnitude."""
    if z.shape[1] > 1:
        top = z.detach().topk(2, dim=1).values
        margins.append(("max", float((top[:, 0] - top[:, 1]).min() / z.detach().abs().max())))


def _clear(v, margins):
    margins.append(("relu", float(v.detach().abs().min() / v.detach().abs().max())))


def restate(kind, shape, B, N, ins, P, train, margins):
    """The layer on the blocks of tests/pointnet_v1_ref.py.  ins: {name: tensor} in P's dtype; returns the list of outputs."""
    if kind == "transform":
        k = shape
        return [torch.einsum("bni,bij->bnj", ins["rows"][:, :k].reshape(B, N, k), ins["trans"]).reshape(B * N, k)]
    if kind == "conv_bn_max":
        ci, co = shape
        z = V._norm(P, "bn", V._linear(P, "conv", ins["x"][:, :ci].reshape(B, N, ci)), train)
        _lead(z, margins)
        return [V._max_points(z, None, "")]
    if kind == "concat":
        cp, cg, co = shape
        w = P["conv.weight"].reshape(co, -1)
        y = ins["pointfeat"].reshape(B, N, cp) @ w[:, cg:].transpose(0, 1) + (ins["g"] @ w[:, :cg].transpose(0, 1))[:, None, :] + P["conv.bias"]
        v = V._norm(P, "bn", y, train)
        _clear(v, margins)
        return [torch.relu(v).reshape(B * N, co)]
    o = [ins["out%d" % (i + 1)].reshape(B, N, -1) for i in range(4)]                 # densecls_ref.dense_forward from out4 on
    out5 = V._norm(P, "bn5", V._linear(P, "conv5", o[3]), train)
    _lead(out5, margins)
    omax = V._max_points(out5, None, "out5")
    g = torch.cat([omax, ins["label"]], 1)
    w = P["convs1.weight"].reshape(DENSE_CO, -1)
    cg = g.shape[1]
    y = (g @ w[:, :cg].transpose(0, 1))[:, None, :] + P["convs1.bias"]
    k = cg
    for t in o + [out5]:
        y = y + t @ w[:, k:k + t.shape[2]].transpose(0, 1)
        k += t.shape[2]
    v = V._norm(P, "bns1", y, train)
    _clear(v, margins)
    return [omax, torch.relu(v).reshape(B * N, DENSE_CO)]


def run_restatement(kind, shape, B, N, S, dtype, device, train, need, layout):
    """One forward / backward of the restatement; returns ({name: tensor}, margins)."""
    P = V.Params(S["sd"], dtype, device)
    ins = {k: v.to(device=device, dtype=dtype).clone().requires_grad_(k in need) for k, v in S["in"].items()}
    margins = []
    outs = restate(kind, shape, B, N, ins, P, train, margins)
    sum(upstream(o, layout, g.to(device)) for o, g in zip(outs, S["gw"])).backward()
    res = {"out%d" % i: o.detach() for i, o in enumerate(outs)}
    res.update({"d/" + k: v.grad for k, v in ins.items() if k in need})
    res.update({"d/" + k: v for k, v in P.grads().items()})
    res.update({k: v for k, v in P.state.items() if not k.endswith("num_batches_tracked")})
    return res, margins


INPUTS = {"transform": ("rows", "trans"), "conv_bn_max": ("x",), "concat": ("pointfeat", "g"),
          "dense": ("out1", "out2", "out3", "out4", "label")}
NEEDS = {"transform": (("rows", "trans"), ("rows",), ("trans",)), "conv_bn_max": (("x",), ()),
         "concat": (("pointfeat", "g"), ("pointfeat",), ("g",), ()),
         "dense": (("out1", "out2", "out3", "out4", "label"), ("out1", "out2", "out3", "out4"))}
KIND_SHAPES = {"transform": (3, 5, 64), "conv_bn_max": ((6, 10), (64, 17)), "concat": ((8, 12, 18),), "dense": (None,)}


@functools.lru_cache(maxsize=None)
def scenario(kind, shape, B, N, train):
    """The operands of a scenario: the first seed from its base whose fp64 restatement clears MARGIN at every decision."""
    base = 1000 * (1 + list(INPUTS).index(kind)) + 100 * KIND_SHAPES[kind].index(shape) + 10 * B + N % 10 + (5 if train else 0)
    for seed in range(base, base + 200):
        S = draw(kind, shape, B, N, seed)
        _, margins = run_restatement(kind, shape, B, N, S, torch.float64, "cpu", train, INPUTS[kind], "contiguous")
        if all(m > MARGIN for _, m in margins):
            S["seed"], S["margins"] = seed, margins
            return S
    raise AssertionError("no seed clears the decision margins")


def cases():
    """(kind, shape, B, N, train, need, layout): every (shape, mode, subset, layout) of a function, (B, N) cycling through SHAPES."""
    out = []
    for kind in INPUTS:
        for i, shape in enumerate(KIND_SHAPES[kind]):
            for train in ((True,) if kind == "transform" else (True, False)):
                for j, need in enumerate(NEEDS[kind]):
                    for l, layout in enumerate(LAYOUTS):
                        B, N = SHAPES[(i + int(train) + j + l) % 4]      # (the shapes rotate against subsets and layouts)
                        out.append((kind, shape, B, N, train, need, layout))
    return out


def _id(c):
    kind, shape, B, N, train, need, layout = c
    return "%s %s B=%d N=%d %s grad=%s upstream=%s" % (kind, shape, B, N, "train" if train else "eval", "+".join(need) or "params-only", layout)


# ------------------------------------------------------------------------------------------------ the library

class _Head(nn.Module):
    """What dense_seg_head reads of a PointNetDenseCls: conv1 .. conv4 (their widths), conv5 / bn5, convs1 / bns1."""

    def __init__(self):
        super().__init__()
        w = (3,) + DENSE_WIDTHS
        for i in range(4):
            setattr(self, "conv%d" % (i + 1), nn.Conv1d(w[i], w[i + 1], 1))
        self.conv5, self.bn5 = nn.Conv1d(w[4], DENSE_C5, 1), nn.BatchNorm1d(DENSE_C5)
        self.convs1 = nn.Conv1d(DENSE_C5 + DENSE_CAT + sum(DENSE_WIDTHS) + DENSE_C5, DENSE_CO, 1)
        self.bns1 = nn.BatchNorm1d(DENSE_CO)


class _Layer(nn.Module):
    def __init__(self, ci, co):
        super().__init__()
        self.conv, self.bn = nn.Conv1d(ci, co, 1), nn.BatchNorm1d(co)


def run_library(kind, shape, B, N, S, dev, train, need, layout):
    from pointnet12_amd import pointnet as M
    ins = {k: v.to(dev).clone().requires_grad_(k in need) for k, v in S["in"].items()}
    net = None
    if kind != "transform":
        net = _Head() if kind == "dense" else _Layer(S["sd"]["conv.weight"].shape[1], S["sd"]["conv.weight"].shape[0])
        net.load_state_dict(S["sd"], strict=False)
        net.to(dev).train(train)
    if kind == "transform":
        outs = [M.point_transform(ins["rows"], ins["trans"], B, N, shape)[:, :shape]]
    elif kind == "conv_bn_max":
        outs = [M.conv_bn_max(ins["x"], net.conv, net.bn, N, train)]
    elif kind == "concat":
        outs = [M.global_concat_conv(ins["pointfeat"], ins["g"], net.conv, net.bn, N, train)]
    else:
        outs = list(M.dense_seg_head(ins["out1"], ins["out2"], ins["out3"], ins["out4"], ins["label"], net, N, train))
    sum(upstream(o, layout, g.to(dev)) for o, g in zip(outs, S["gw"])).backward()
    res = {"out%d" % i: o.detach() for i, o in enumerate(outs)}
    for k, v in ins.items():
        if k in need:
            c = shape if k == "rows" else shape[0] if k == "x" else v.shape[-1]
            res["d/" + k] = v.grad[..., :c]                          # (the real columns of a padded input)
        else:
            assert v.grad is None, k
    if net is not None:
        res.update({"d/" + k: p.grad for k, p in net.named_parameters() if k in S["sd"]})
        res.update({k: b for k, b in net.named_buffers() if k in S["sd"] and not k.endswith("num_batches_tracked")})
        for k, b in net.named_buffers():
            if k.endswith("num_batches_tracked") and k in S["sd"]:
                assert int(b) == int(train), k
    return res


def _ref_cols(kind, shape, k, t):
    """The restatement differentiates the padded inputs too: only the real columns are compared."""
    if k == "d/rows":
        return t[:, :shape]
    if k == "d/x":
        return t[:, :shape[0]]
    return t


@pytest.mark.parametrize("case", cases(), ids=_id)
def test_layer_against_fp64(dev, case):
    kind, shape, B, N, train, need, layout = case
    S = scenario(kind, shape, B, N, train)
    ref, _ = run_restatement(kind, shape, B, N, S, torch.float64, dev, train, need, layout)
    f32, _ = run_restatement(kind, shape, B, N, S, torch.float32, dev, train, need, layout)
    got = run_library(kind, shape, B, N, S, dev, train, need, layout)
    assert sorted(got) == sorted(ref), (sorted(got), sorted(ref))
    bad = []
    for k, r in ref.items():
        r, f, g = _ref_cols(kind, shape, k, r), _ref_cols(kind, shape, k, f32[k]), got[k]
        assert g.shape == r.shape, (k, g.shape, r.shape)
        scale = float(r.abs().max())
        if train and k.endswith(("conv.bias", "conv5.bias", "convs1.bias")) and k.startswith("d/"):
            scale = float(ref[k[:-len("bias")] + "weight"].abs().max())           # bias before a training-mode BatchNorm: exactly 0
        err, err32 = float((g.double() - r).abs().max()), float((f.double() - r).abs().max())
        if not err <= max(3e-5 * scale, 4.0 * err32):
            bad.append((k, err, err32, scale))
    assert not bad, "seed %d: %s" % (S["seed"], bad)
