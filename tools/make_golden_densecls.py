#!/usr/bin/env python3
"""Generate tests/golden/g14_densecls.npz by running the REFERENCE's PointNetDenseCls and PointNetLoss (model/pointnet.py, imported
unmodified) on CPU (development container only, like tools/make_golden_pointnet.py).  Only numbers the reference computed are written:

  <Net>/keys, /shapes, /dtypes, /sha256, /args   the seeded (torch.manual_seed(0)) state_dict of PointNetDenseCls() and
                                                 PointNetDenseCls(5, 7)
  step/*                                         one training step of PointNetDenseCls() at B = 8 x N = 500 (train mode, dropout off)
                                                 with PointNetLoss(weight=0.5), so that the classification head's gradient reaches
                                                 out_max beside the segmentation head's: inputs, net, net2, trans, trans_feat, the
                                                 three losses (and loss1/*: the same outputs under the default weight = 1), the input
                                                 gradient, every parameter gradient (tensors above SLICE_MIN elements as their first
                                                 SLICE_ROWS rows, with the full tensor's largest |entry| as <key>/absmax), the running
                                                 statistics after the step, the eval-mode outputs after it, and noise/<key>: the
                                                 largest |difference| of each recorded tensor between 8-thread and 1-thread runs.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_densecls.py
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("PN2_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

from model import pointnet as R          # noqa: E402  (the reference)

OUT = os.path.join(ROOT, "tests", "golden", "g14_densecls.npz")
B, N, CATS, PARTS = 8, 500, 16, 50
SLICE_MIN, SLICE_ROWS = 4096, 1
STATE_NETS = (("PointNetDenseCls", ()), ("PointNetDenseCls_5_7", (5, 7)))


def state_digest(module):
    h = hashlib.sha256()
    for k, v in module.state_dict().items():
        h.update(k.encode())
        h.update(v.detach().numpy().tobytes())
    return h.hexdigest()


def record(out, key, t):
    a = t.detach().numpy().astype(np.float32)
    if a.size > SLICE_MIN:
        out[key + "/absmax"] = np.float32(np.abs(a).max())
        a = a[:SLICE_ROWS]
    out[key] = np.ascontiguousarray(a)


def step(threads):
    """One training step of the reference net on fixed inputs; returns {key: array} of everything recorded."""
    torch.set_num_threads(threads)
    torch.manual_seed(0)
    net = R.PointNetDenseCls()
    net.train()
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.eval()
    gen = torch.Generator().manual_seed(15)
    x = torch.randn(B, 3, N, generator=gen)
    cls = torch.randint(0, CATS, (B,), generator=gen)
    seg = torch.randint(0, PARTS, (B, N), generator=gen)
    onehot = torch.eye(CATS)[cls]                    # utils.to_categorical of the reference's driver
    x.requires_grad_(True)
    seen = {}
    hook = net.stn.register_forward_hook(lambda m, i, o: seen.__setitem__("trans", o))
    labels_pred, seg_pred, trans_feat = net(x, onehot)
    hook.remove()
    flat, target = seg_pred.contiguous().view(-1, PARTS), seg.view(-1)
    loss, seg_loss, label_loss = R.PointNetLoss(weight=0.5)(labels_pred, cls, flat, target, trans_feat)
    loss1, seg_loss1, label_loss1 = R.PointNetLoss()(labels_pred, cls, flat, target, trans_feat)
    loss.backward()
    out = {"x": x.detach().numpy().copy(), "cls": cls.numpy().astype(np.int64), "seg": seg.numpy().astype(np.int64)}
    record(out, "net", labels_pred)
    record(out, "net2", seg_pred)
    record(out, "trans", seen["trans"])
    record(out, "trans_feat", trans_feat)
    for k, v in (("loss", loss), ("seg_loss", seg_loss), ("label_loss", label_loss), ("loss1/loss", loss1), ("loss1/seg_loss", seg_loss1),
                 ("loss1/label_loss", label_loss1)):
        out[k] = np.float64(v.item())
    record(out, "grad/x", x.grad)
    for k, p in net.named_parameters():
        record(out, "grad/" + k, p.grad)
    for k, v in net.state_dict().items():
        if k.endswith(("running_mean", "running_var")):
            record(out, "after/" + k, v)
    net.eval()
    with torch.no_grad():
        n_e, n2_e, tf_e = net(x.detach(), onehot)
    record(out, "eval/net", n_e)
    record(out, "eval/net2", n2_e)
    record(out, "eval/trans_feat", tf_e)
    torch.set_num_threads(8)
    return out


def main():
    out = {}
    for name, args in STATE_NETS:
        torch.manual_seed(0)
        net = R.PointNetDenseCls(*args)
        sd = net.state_dict()
        out[name + "/args"] = np.array([int(a) for a in args], np.int64)
        out[name + "/keys"] = np.array(list(sd))
        out[name + "/shapes"] = np.array(["x".join(map(str, v.shape)) for v in sd.values()])
        out[name + "/dtypes"] = np.array([str(v.dtype) for v in sd.values()])
        out[name + "/sha256"] = np.array(state_digest(net))
        print("  %s: %d tensors" % (name, len(sd)))
    a, b = step(8), step(1)
    for k, v in a.items():
        out["step/" + k] = v
        if k not in ("x", "cls", "seg") and not k.endswith("/absmax"):
            out["step/noise/" + k] = np.float64(np.abs(np.asarray(v, np.float64) - np.asarray(b[k], np.float64)).max())
    print("  step: loss %.6f, worst thread noise %.2e" % (a["loss"], max(v for k, v in out.items() if k.startswith("step/noise/"))))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%.1f KB)" % (OUT, os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
