#!/usr/bin/env python3
"""Generate tests/golden/g13_pointnet.npz by running the REFERENCE's PointNet v1 (model/pointnet.py, imported unmodified) on CPU
(development container only, like tools/make_golden*.py).  Only numbers the reference computed are written:

  <Net>/keys, /shapes, /dtypes, /sha256, /args   the seeded (torch.manual_seed(0)) state_dict of STN3d(), STNkd(64),
                                                 PointNetCls(40, True / False), PointNetSeg(13, 9, True), PointNetSeg(19, 4, True)
  seg/*, cls/*                                   one training step of PointNetSeg(13, 9, True) and PointNetCls(40, True) at
                                                 B = 8 x N = 500 (train mode, dropout off): input, outputs, trans, trans_feat, the
                                                 loss nll + 0.001 reg, the input gradient, every parameter gradient (tensors above
                                                 SLICE_MIN elements as their first SLICE_ROWS rows, with the full tensor's largest
                                                 |entry| as <key>/absmax), the running statistics after the step, the eval-mode
                                                 outputs after it, and noise/<key>: the largest |difference| of each recorded tensor
                                                 between 8-thread and 1-thread runs of the reference (the g6_noise idea).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_pointnet.py
"""
import hashlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("PN2_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

from model import pointnet as R          # noqa: E402  (the reference)

OUT = os.path.join(ROOT, "tests", "golden", "g13_pointnet.npz")
B, N = 8, 500
SLICE_MIN, SLICE_ROWS = 4096, 2
STATE_NETS = (("STN3d", ()), ("STNkd", (64,)), ("PointNetCls", (40, True)), ("PointNetCls_noft", (40, False)),
              ("PointNetSeg", (13, 9, True)), ("PointNetSeg_kitti", (19, 4, True)))


def state_digest(module):
    h = hashlib.sha256()
    for k, v in module.state_dict().items():
        h.update(k.encode())
        h.update(v.detach().numpy().tobytes())
    return h.hexdigest()


def make(name, args):
    return getattr(R, name.split("_")[0])(*args)


def record(out, key, t):
    a = t.detach().numpy().astype(np.float32)
    if a.size > SLICE_MIN:
        out[key + "/absmax"] = np.float32(np.abs(a).max())
        a = a[:SLICE_ROWS]
    out[key] = np.ascontiguousarray(a)


def step(tag, threads):
    """One training step of the reference net on fixed inputs; returns {key: array} of everything recorded."""
    torch.set_num_threads(threads)
    torch.manual_seed(0)
    if tag == "seg":
        net, C, classes = R.PointNetSeg(13, 9, True), 9, 13
    else:
        net, C, classes = R.PointNetCls(40, True), 3, 40
    net.train()
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.eval()
    gen = torch.Generator().manual_seed(13 if tag == "seg" else 14)
    x = torch.randn(B, C, N, generator=gen)
    labels = torch.randint(0, classes, (B, N) if tag == "seg" else (B,), generator=gen)
    x.requires_grad_(True)
    seen = {}
    hook = net.feat.stn.register_forward_hook(lambda m, i, o: seen.__setitem__("trans", o))
    lp, trans_feat = net(x)
    hook.remove()
    nll = F.nll_loss(lp.reshape(-1, classes), labels.reshape(-1))
    reg = R.feature_transform_reguliarzer(trans_feat)
    loss = nll + 0.001 * reg
    loss.backward()
    out = {"x": x.detach().numpy().copy(), "labels": labels.numpy().astype(np.int64)}
    record(out, "log_probs", lp)
    record(out, "trans", seen["trans"])
    record(out, "trans_feat", trans_feat)
    out["loss"] = np.float64(loss.item())
    out["reg"] = np.float64(reg.item())
    out["reg_slice"] = np.float64(R.feature_transform_reguliarzer(trans_feat[:SLICE_ROWS]).item())    # (of the recorded clouds)
    record(out, "grad/x", x.grad)
    for k, p in net.named_parameters():
        record(out, "grad/" + k, p.grad)
    for k, v in net.state_dict().items():
        if k.endswith(("running_mean", "running_var")):
            record(out, "after/" + k, v)
    net.eval()
    with torch.no_grad():
        lp_e, tf_e = net(x.detach())
    record(out, "eval/log_probs", lp_e)
    record(out, "eval/trans_feat", tf_e)
    torch.set_num_threads(8)
    return out


def main():
    out = {}
    for name, args in STATE_NETS:
        torch.manual_seed(0)
        net = make(name, args)
        sd = net.state_dict()
        out[name + "/args"] = np.array([int(a) for a in args], np.int64)
        out[name + "/keys"] = np.array(list(sd))
        out[name + "/shapes"] = np.array(["x".join(map(str, v.shape)) for v in sd.values()])
        out[name + "/dtypes"] = np.array([str(v.dtype) for v in sd.values()])
        out[name + "/sha256"] = np.array(state_digest(net))
        print("  %s: %d tensors" % (name, len(sd)))
    for tag in ("seg", "cls"):
        a, b = step(tag, 8), step(tag, 1)
        for k, v in a.items():
            out[tag + "/" + k] = v
            if k not in ("x", "labels") and not k.endswith("/absmax"):
                out[tag + "/noise/" + k] = np.float64(np.abs(np.asarray(v, np.float64) - np.asarray(b[k], np.float64)).max())
        print("  %s: loss %.6f, worst thread noise %.2e" % (tag, a["loss"], max(out[tag + "/noise/" + k] for k in a
                                                                                  if (tag + "/noise/" + k) in out)))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%.1f KB)" % (OUT, os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
