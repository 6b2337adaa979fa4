#!/usr/bin/env python
"""Launch trace of the Python glue around the shared-MLP kernels: which C-ABI calls a fixed list of small seeded scenarios makes.

    python tools/launch_trace.py out.json

For every scenario (forward + backward, two consecutive steps: ``_PAIR_RUNS_SPLIT`` makes the second differ from the first) the file
holds, per C-ABI call in issue order, the entry name as ``_lib.call_profile`` books it (``pn2_conv1x1_bwd_pair_split`` is a name of
its own), every integer argument below 2^31 verbatim, every pointer argument as "null" / "ptr", and the ``pn2_last_kernel()`` name;
and a SHA-256 of each step's forward outputs.  Two trees whose glue issues the same calls write the same file: a refactor of
``pointnet_util.py`` / ``pointnet.py`` is checked by running this at both commits and comparing (``cmp a.json b.json``).

The scenarios cover every entry point that ``_SharedMLP``, ``_Conv1x1`` and the autograd functions of ``pointnet.py`` can call
(``REQUIRED`` below); the run fails if one of them is missing from the trace.
"""
import ctypes
import hashlib
import json
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointnet12_amd import _lib                      # noqa: E402
from pointnet12_amd import pointnet as PN            # noqa: E402
from pointnet12_amd import pointnet_util as U        # noqa: E402

REQUIRED = """pn2_group_conv_fwd pn2_group_affine_fwd pn2_conv1x1_fwd pn2_conv1x1_fwd_pool pn2_copy_cols pn2_bn_finalize
pn2_bn_pool_select pn2_bn_relu_max pn2_pool_bwd_reduce_rec pn2_pool_bwd_reduce_ld pn2_relu_bwd_reduce pn2_bn_bwd_coef
pn2_conv1x1_bwd_first pn2_conv1x1_wgrad_cf pn2_conv1x1_wgrad_cf/no_dz pn2_conv1x1_bwd_cf pn2_conv1x1_bwd pn2_conv1x1_bwd_pair
pn2_conv1x1_bwd_pair_split pn2_conv1x1_dgrad pn2_conv1x1_wgrad pn2_conv1x1_wgrad_ws pn2_group_bwd pn2_group_affine_bwd_seg
pn2_group_affine_bwd pn2_bn_max pn2_pool_bwd_reduce_noact pn2_conv1x1_fwd_gbias pn2_group_colsum pn2_conv1x1_fwd_multi
pn2_conv1x1_wgrad_multi pn2_conv1x1_dgrad_multi pn2_bn_bwd_reduce_noact_dense pn2_point_transform pn2_point_transform_bwd""".split()

DEV = torch.device("cuda:0")
_modules = []            # what the scenario being built owns parameters in: their gradients are dropped between its two steps


def _arg(a, ctype):
    if ctype is ctypes.c_void_p:
        return "null" if a is None or a == 0 else "ptr"
    if isinstance(a, float):
        return repr(a)
    a = int(a)
    return a if -(1 << 31) <= a < (1 << 31) else "big"


def _call(c):
    name, args, _, _, kern = c
    types = _lib.SIGNATURES[name[:-6] if name.endswith("_split") else name][1]
    return [name, [_arg(a, t) for a, t in zip(args[:-1], types[:-1])], kern]      # (the last argument is the stream handle)


def _tensors(v):
    if isinstance(v, torch.Tensor):
        return [v]
    if isinstance(v, (tuple, list)):
        return [t for x in v for t in _tensors(x)]
    return []


def _trace(fn, direct, steps=2):
    """fn() -> output tensor(s); backward of a fixed random weighting of the outputs that carry a gradient."""
    U._PAIR_RUNS_SPLIT.clear()
    calls, hashes = [], []
    for step in range(steps):
        if not direct:               # (as optimizer.zero_grad(set_to_none=True); direct accumulation keeps its .grad tensors)
            for m in _modules:
                for p in m.parameters():
                    p.grad = None
        torch.manual_seed(100 + step)
        with _lib.call_profile() as prof:
            outs = _tensors(fn())
            loss = None
            for i, o in enumerate(outs):
                if o.requires_grad and o.is_floating_point():
                    gw = torch.randn(o.shape, generator=torch.Generator().manual_seed(7 + i)).to(DEV)
                    loss = (o * gw).sum() if loss is None else loss + (o * gw).sum()
            loss.backward()
            torch.cuda.synchronize()
            calls.append([_call(c) for c in prof])
        h = hashlib.sha256()
        for o in outs:
            h.update(o.detach().contiguous().cpu().numpy().tobytes())
        hashes.append(h.hexdigest())
    return {"calls": calls, "forward_sha256": hashes}


def _stack(chans, seed, two_d=True):
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    convs = nn.ModuleList([(nn.Conv2d if two_d else nn.Conv1d)(a, b, 1) for a, b in zip(chans[:-1], chans[1:])])
    bns = nn.ModuleList([(nn.BatchNorm2d if two_d else nn.BatchNorm1d)(b) for b in chans[1:]])
    for bn in bns:
        bn.weight.data.uniform_(0.5, 1.5, generator=gen)
        bn.bias.data.uniform_(-0.5, 0.5, generator=gen)
    _modules.extend([convs, bns])
    return convs.to(DEV), bns.to(DEV)


def mlp(P, pool, chans, training=True, need_dx=True, direct=False):
    """shared_mlp on plain rows [P, round4(chans[0])]."""
    c_in = chans[0]
    gen = torch.Generator().manual_seed(P + pool + c_in)
    rows = torch.zeros(P, (c_in + 3) & ~3)
    rows[:, :c_in] = torch.randn(P, c_in, generator=gen) * 2 + 0.5
    convs, bns = _stack(chans, P + pool)
    x = rows.to(DEV).requires_grad_(need_dx)
    if direct:
        for p in list(convs.parameters()) + list(bns.parameters()):
            p.grad = torch.zeros_like(p)
    return lambda: U.shared_mlp(x, c_in, convs, bns, pool, training)


def _cloud(B, N, D, seed, feat_grad=False):
    gen = torch.Generator().manual_seed(seed)
    xyz = (torch.rand(B, 3, N, generator=gen) * 2 - 1).to(DEV)
    feat = torch.randn(B, D, N, generator=gen).to(DEV).requires_grad_(feat_grad) if D else None
    return xyz, feat


def sa(S, radius, K, c_in, chans, B, N, feat_grad=False, group_all=False, direct=False):
    xyz, feat = _cloud(B, N, c_in - 3, S or 1, feat_grad)
    torch.manual_seed(7)
    mod = U.PointNetSetAbstraction(S, radius, K, c_in, chans, group_all).to(DEV).train()
    _modules.append(mod)
    if direct:
        for p in mod.parameters():
            p.grad = torch.zeros_like(p)
    return lambda: mod(xyz, feat)[1]


def msg(B, N):
    xyz, feat = _cloud(B, N, 6, 5, True)
    torch.manual_seed(7)
    mod = U.PointNetSetAbstractionMsg(64, [0.2, 0.4, 0.8], [16, 32, 128], 6, [[16, 32], [32, 48, 64], [32, 196]]).to(DEV).train()
    _modules.append(mod)
    return lambda: mod(xyz, feat)[1]


def fp(B, N, S):
    xyz, feat = _cloud(B, N, 6, 9, True)
    p2 = torch.randn(B, 24, S, generator=torch.Generator().manual_seed(8)).to(DEV).requires_grad_(True)
    x2 = xyz[:, :, :S].contiguous() if S > 1 else torch.zeros(B, 3, 1, device=DEV)
    torch.manual_seed(7)
    mod = U.PointNetFeaturePropagation(6 + 24, [40, 16]).to(DEV).train()
    _modules.append(mod)
    return lambda: mod(xyz, x2, feat, p2)


def classifier(P, ci, co):
    torch.manual_seed(P + ci)
    conv = nn.Conv1d(ci, co, 1).to(DEV)
    _modules.append(conv)
    x = torch.randn(P, ci, device=DEV).requires_grad_(True)
    return lambda: U.log_softmax_rows(U.conv1x1(x, conv, padded=True), co)


def network(kind, B=2, N=256):
    torch.manual_seed(3)
    gen = torch.Generator().manual_seed(4)
    if kind == "cls":
        net, args = PN.PointNetCls(k=40, feature_transform=True), (torch.randn(B, 3, N, generator=gen),)
    elif kind == "seg":
        net, args = PN.PointNetSeg(13, input_dims=4, feature_transform=True), (torch.randn(B, 4, N, generator=gen),)
    else:
        label = torch.zeros(B, 16)
        label[torch.arange(B), torch.arange(B) % 16] = 1.0
        net, args = PN.PointNetDenseCls(16, 50), (torch.randn(B, 3, N, generator=gen), label)
    net.to(DEV).train()
    _modules.append(net)
    args = tuple(a.to(DEV) for a in args)
    return lambda: net(*args)


class _patched:
    """Module attributes of pointnet_util / library options / direct accumulation set for one scenario, restored after it."""

    def __init__(self, attrs=None, options=None, direct=False):
        self.attrs, self.options, self.direct = attrs or {}, options or {}, direct

    def __enter__(self):
        self.old_attrs = {k: getattr(U, k) for k in self.attrs}
        self.old_options = {k: _lib.options()[k] for k in self.options}
        for k, v in self.attrs.items():
            setattr(U, k, v)
        for k, v in self.options.items():
            _lib.set_option(k, v)
        U.set_direct_grad_accumulation(self.direct)

    def __exit__(self, *exc):
        for k, v in self.old_attrs.items():
            setattr(U, k, v)
        for k, v in self.old_options.items():
            _lib.set_option(k, v)
        U.set_direct_grad_accumulation(False)
        return False


SA1 = dict(S=512, radius=0.4, K=128, c_in=9, chans=[64, 96, 128], B=4, N=4096)        # gather-conv first layer, from-input last layer

# name -> (builder, keyword arguments of _patched)
SCENARIOS = [
    ("pooled_64_96_128_k16", lambda: mlp(65536, 16, [64, 96, 128]), {}),
    ("pooled_32_64_64_k64_ragged", lambda: mlp(32768 + 64, 64, [32, 64, 64]), {}),
    ("pooled_64_128_256_k128", lambda: mlp(65536, 128, [64, 128, 256]), {}),
    ("pair_few_rows_k128", lambda: mlp(2048, 128, [256, 256, 512, 1024]), {}),
    ("pair_dense_576", lambda: mlp(8192, 0, [576, 256, 128]), {}),
    ("pair_128x128", lambda: mlp(8192, 0, [128, 128, 128]), {}),
    ("wide_259_k32", lambda: mlp(4096, 32, [259, 256, 256, 512]), {}),
    ("wide_196_256_k128", lambda: mlp(131072, 128, [64, 196, 256]), {}),
    ("wide_196_256_k128_two_phase_wgrad", lambda: mlp(131072, 128, [64, 196, 256]), dict(options={"PN2_WGRAD_TWO_PHASE": 1})),
    ("dense_long_64_96", lambda: mlp(300000, 0, [64, 96]), {}),
    ("first_layer_no_dx_cf", lambda: mlp(8192, 0, [12, 96], need_dx=False), {}),
    ("first_layer_no_dx_wide", lambda: mlp(40001, 0, [20, 64, 32], need_dx=False), {}),
    ("sa1", lambda: sa(**SA1), {}),
    ("sa1_fuse_first", lambda: sa(**SA1), dict(options={"PN2_FUSE_FIRST": 1})),
    ("sa1_dx", lambda: sa(feat_grad=True, **SA1), {}),
    ("factorised", lambda: sa(64, 0.4, 32, 35, [64, 64], 2, 1024, feat_grad=True), {}),
    ("factorised_no_gather_bwd", lambda: sa(64, 0.4, 32, 35, [64, 64], 2, 1024, feat_grad=True), dict(attrs={"GATHER_BACKWARD": False})),
    ("factorised_d33_no_dx", lambda: sa(64, 0.4, 32, 36, [48, 64], 2, 1024), {}),
    ("msg", lambda: msg(2, 1024), {}),
    ("group_all", lambda: sa(None, None, None, 9, [64, 256, 520], 2, 128, feat_grad=True, group_all=True), {}),
    ("fp_s1", lambda: fp(2, 1024, 1), {}),
    ("fp_s128", lambda: fp(2, 1024, 128), {}),
    ("aligned_weight_137", lambda: mlp(32768, 0, [137, 128, 128]), {}),
    ("eval_bn_dense", lambda: mlp(5000, 0, [5, 80, 32], training=False), {}),
    ("eval_bn_pooled", lambda: mlp(4096, 32, [9, 32, 64], training=False), {}),
    ("direct_grads", lambda: mlp(32768 + 64, 64, [32, 64, 64], direct=True), dict(direct=True)),
    ("direct_grads_sa1", lambda: sa(direct=True, **SA1), dict(direct=True)),
    ("no_lazy_bn", lambda: mlp(32768 + 64, 64, [32, 64, 64]), dict(attrs={"LAZY_BN": False})),
    ("no_lazy_bn_sa1", lambda: sa(**SA1), dict(attrs={"LAZY_BN": False})),
    ("no_bwd_pair", lambda: mlp(8192, 0, [576, 256, 128]), dict(attrs={"BWD_PAIR": False})),
    ("no_wgrad_cf", lambda: mlp(8192, 0, [12, 96], need_dx=False), dict(attrs={"WGRAD_CF": False})),
    ("no_pool_in_epilogue", lambda: mlp(65536, 16, [64, 96, 128]), dict(attrs={"POOL_IN_EPILOGUE": False})),
    ("no_gather_conv", lambda: sa(**SA1), dict(attrs={"GATHER_CONV": False})),
    ("classifier_padded_log_softmax", lambda: classifier(9000, 128, 13), {}),
    ("pointnet_cls", lambda: network("cls"), {}),
    ("pointnet_seg", lambda: network("seg"), {}),
    ("pointnet_dense_cls", lambda: network("dense"), {}),
]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else "launch_trace.json"
    only = sys.argv[2:]
    result = {}
    for name, build, patch in SCENARIOS:
        if only and name not in only:
            continue
        del _modules[:]
        with _patched(**patch):
            result[name] = _trace(build(), patch.get("direct", False))
        print("%-32s %4d + %4d calls" % (name, len(result[name]["calls"][0]), len(result[name]["calls"][1])), flush=True)
    seen = set()
    for r in result.values():
        for step in r["calls"]:
            for name, args, _ in step:
                seen.add(name)
                if name == "pn2_conv1x1_wgrad_cf" and args[0] == "null":
                    seen.add("pn2_conv1x1_wgrad_cf/no_dz")
    with open(out_path, "w") as f:
        json.dump(result, f, indent=0, sort_keys=True)
        f.write("\n")
    missing = [n for n in REQUIRED if n not in seen]
    if missing and not only:
        print("entry points the trace does not reach: " + " ".join(missing))
        return 1
    print("wrote %s: %d scenarios, %d entry points" % (out_path, len(result), len(seen)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
