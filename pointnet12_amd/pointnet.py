"""MI355X-native counterpart of the reference's ``model/pointnet.py`` (PointNet v1).

Same class names, constructor arguments, attribute names and registration order as the reference (``STN3d``, ``STNkd``,
``PointNetEncoder``, ``PointNetCls``, ``PointNetSeg``, ``PointNetDenseCls``, ``PointNetLoss``, ``feature_transform_reguliarzer``), so
``state_dict`` keys, shapes and seeded initial values are the reference's and its checkpoints load with
``pointnet2.load_reference_state``.

Every per-point operation runs on the HIP library: the conv + BatchNorm + ReLU stacks (the STN stacks pooled over the whole
cloud included) through ``shared_mlp``, ``torch.bmm(x, trans)`` through ``pn2_point_transform``, the encoder's conv3 + bn3 + max
(no ReLU) through ``pn2_bn_max``, and the segmentation head's conv1 over ``cat([global.repeat(N), pointfeat])`` factorised as
``W_p pointfeat_p + b + W_g g_b`` -- the [B*N, 1088] concatenation never exists.  Work on [B, .] vectors (the STN fully
connected layers, the classification head, the regulariser) stays stock PyTorch, as the PointNet++ classification head does.
"""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import check as _check, ptr as _p
from .loss import nll_loss
from .pointnet_util import (_REPL, _UpGrad, _carve, _channel_last, _contig_weight, _empty_rows, _gpu_f32, _r4,
                            bump_param_generation, conv1x1, log_softmax_rows, shared_mlp)


def _rows(x):
    """[B, C, N] channel-first -> position-major rows [B*N, round4(C)] with zero pad columns."""
    B, C, N = x.shape
    r = _channel_last(x, "x").reshape(B * N, C)
    if C % 4:
        r = F.pad(r, (0, _r4(C) - C))
    return r


def _bn_cfg(bn):
    if bn.momentum is None:
        raise NotImplementedError("cumulative-average BatchNorm (momentum=None) is not supported")
    return float(bn.eps), float(bn.momentum)


class _PointTransform(torch.autograd.Function):
    """rows [B*N, round4(k)] -> rows @ trans[b] per cloud (torch.bmm(x.transpose(2, 1), trans) of the reference)."""

    @staticmethod
    def forward(ctx, rows, trans, B, N, k):
        lib, st = _lib.load(), _lib.stream()
        out = _empty_rows(B * N, k, rows.device)
        _check(lib.pn2_point_transform(_p(rows), rows.shape[1], _p(trans), B, N, k, _p(out), out.shape[1], st), "pn2_point_transform")
        ctx.save_for_backward(rows, trans)
        ctx.dims = (B, N, k)
        return out

    @staticmethod
    def backward(ctx, grad):
        lib, st = _lib.load(), _lib.stream()
        rows, trans = ctx.saved_tensors
        B, N, k = ctx.dims
        kp = _r4(k)
        grad = grad.contiguous()
        if grad.shape[1] != kp:
            grad = F.pad(grad, (0, kp - grad.shape[1]))
        dx = torch.empty(B * N, rows.shape[1], device=rows.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        dT = torch.empty(B, k, k, device=rows.device, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        if dx is None and dT is None:
            return None, None, None, None, None
        ws = None
        if dT is not None:
            ws = torch.empty(int(lib.pn2_point_transform_workspace_bytes(B, N, k)), device=rows.device, dtype=torch.uint8)
        _check(lib.pn2_point_transform_bwd(_p(grad), grad.shape[1], _p(rows), rows.shape[1], _p(trans), B, N, k, _p(dx),
                                           rows.shape[1], _p(dT), _p(ws), st), "pn2_point_transform_bwd")
        return dx, dT, None, None, None


def point_transform(rows, trans, B, N, k):
    """Apply the per-cloud k x k matrix ``trans`` [B, k, k] to every row of ``rows`` [B*N, round4(k)] (HIP)."""
    rows = _gpu_f32(rows, "rows")
    if rows.shape != (B * N, _r4(k)):
        raise RuntimeError("rows must be [B*N, round4(k)] with zero pad columns")
    if trans.shape != (B, k, k):
        raise RuntimeError("trans must be [B, k, k]")
    return _PointTransform.apply(rows, _gpu_f32(trans, "trans"), B, N, k)


class _ConvBnMax(torch.autograd.Function):
    """max over the N points of a cloud of bn(conv(x)) -- conv3 + bn3 + torch.max of PointNetEncoder, no ReLU."""

    @staticmethod
    def forward(ctx, x, N, training, cfg, w, b, gamma, beta, rmean, rvar, nbt):
        lib, st = _lib.load(), _lib.stream()
        dev = x.device
        P, ldx = x.shape
        co, ci = w.shape[0], w.shape[1]
        G = P // N
        eps, mom = cfg
        stats, aff = _carve(dev, [(torch.float64, _REPL * 2 * co), (torch.float32, 4 * _r4(co))])
        y = _empty_rows(P, co, dev)
        _check(lib.pn2_conv1x1_fwd(_p(x), ldx, None, _p(_contig_weight(w)), ci, _p(b), _p(y), y.shape[1], P, ci, co,
                                   _p(stats) if training else None, None, st), "pn2_conv1x1_fwd")
        _check(lib.pn2_bn_finalize(_p(stats), P, co, _p(gamma), _p(beta), eps, mom, int(training), _p(rmean), _p(rvar), _p(nbt),
                                   _p(aff), st), "pn2_bn_finalize")
        out = _empty_rows(G, co, dev)
        arg = torch.empty(G, out.shape[1], device=dev, dtype=torch.int32)
        _check(lib.pn2_bn_max(_p(y), y.shape[1], _p(aff), G, N, co, _p(out), out.shape[1], _p(arg), st), "pn2_bn_max")
        if training:
            bump_param_generation()             # running statistics were written through raw pointers
        ctx.save_for_backward(x, y, aff, arg, w, gamma)
        ctx.meta = (N, bool(training), P, G, co, ci)
        ctx.params = (w, b)
        return out[:, :co] if out.shape[1] != co else out

    @staticmethod
    def backward(ctx, grad):
        lib, st = _lib.load(), _lib.stream()
        x, y, aff, arg, w, gamma = ctx.saved_tensors
        N, training, P, G, co, ci = ctx.meta
        dev = x.device
        ldo = arg.shape[1]
        if grad.stride(-1) != 1 or grad.stride(0) < co or grad.dtype != torch.float32:     # (a row-broadcast gradient, as .sum(0)
            grad = grad.contiguous().float()                                                # hands back, has pitch 0)
        red, coef, dW, db = _carve(dev, [(torch.float64, _REPL * 2 * co), (torch.float32, 4 * _r4(co)), (torch.float32, co * ci),
                                         (torch.float32, co)])
        dW = dW.view(co, ci)
        dzp = torch.empty(G, ldo, device=dev, dtype=torch.float32)
        _check(lib.pn2_pool_bwd_reduce_noact(_p(grad), grad.stride(0), _p(arg), ldo, _p(y), y.shape[1], _p(aff), G, N, co, _p(dzp),
                                             _p(red), st), "pn2_pool_bwd_reduce_noact")
        dgamma = torch.empty(co, device=dev, dtype=torch.float32)
        dbeta = torch.empty(co, device=dev, dtype=torch.float32)
        _check(lib.pn2_bn_bwd_coef(_p(red), P, co, _p(gamma), _p(aff), int(training), _p(coef), _p(dgamma), _p(dbeta), 0, st),
               "pn2_bn_bwd_coef")
        dy = _UpGrad.pooled(dzp, ldo, arg, N, y, coef)
        _check(lib.pn2_conv1x1_wgrad(*dy, _p(x), x.shape[1], None, _p(dW), ci, None if training else _p(db), P, co, ci, None, st),
               "pn2_conv1x1_wgrad")
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(P, x.shape[1], device=dev, dtype=torch.float32)
            _check(lib.pn2_conv1x1_dgrad(*dy, _p(_contig_weight(w)), ci, None, 0, None, _p(dx), dx.shape[1], None, P, co, ci, None, st),
                   "pn2_conv1x1_dgrad")
        return dx, None, None, None, dW.view_as(w), db, dgamma, dbeta, None, None, None


def conv_bn_max(x, conv, bn, N, training):
    """x [B*N, round4(C_in)] -> max over each cloud's N rows of bn(conv(x)), [B, C_out] (HIP)."""
    x = _gpu_f32(x, "rows")
    if x.shape[0] % N or x.shape[1] != _r4(conv.in_channels):
        raise RuntimeError("rows must be [B*N, round4(C_in)]")
    return _ConvBnMax.apply(x, N, bool(training), _bn_cfg(bn), conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean,
                            bn.running_var, bn.num_batches_tracked)


class _GlobalConcatConv(torch.autograd.Function):
    """relu(bn(conv(cat([g.repeat(N), pointfeat])))) with the conv factorised: y_p = W_p pointfeat_p + b + W_g g_b.

    The weight [C_out, C_g + C_p] is read in place at its own pitch: the global columns by a [B]-row GEMM, the point columns by
    the per-point GEMM (pn2_conv1x1_fwd_gbias).  Backward: the per-point part through the plain data / weight gradient GEMMs, the
    per-cloud part from s_b = sum_{p in b} dY_p (pn2_group_colsum): dW_g = s^T g, dg = s W_g, db = sum_b s_b."""

    @staticmethod
    def forward(ctx, pf, g, N, training, cfg, w, b, gamma, beta, rmean, rvar, nbt):
        lib, st = _lib.load(), _lib.stream()
        dev = pf.device
        P, ldp = pf.shape
        B, cg = g.shape
        co, ct = w.shape[0], w.shape[1]
        cp = ct - cg
        eps, mom = cfg
        wc = _contig_weight(w)
        stats, aff, zero_bias = _carve(dev, [(torch.float64, _REPL * 2 * co), (torch.float32, 4 * _r4(co)), (torch.float32, co)])
        gterm = _empty_rows(B, co, dev)                # W_g g_b: one row per cloud
        _check(lib.pn2_conv1x1_fwd(_p(g), cg, None, _p(wc), ct, _p(zero_bias), _p(gterm), gterm.shape[1], B, cg, co, None, None, st),
               "pn2_conv1x1_fwd")
        y = _empty_rows(P, co, dev)
        _check(lib.pn2_conv1x1_fwd_gbias(_p(pf), ldp, wc.data_ptr() + 4 * cg, ct, _p(b), _p(gterm), gterm.shape[1], N, _p(y), y.shape[1],
                                         P, cp, co, _p(stats) if training else None, st), "pn2_conv1x1_fwd_gbias")
        _check(lib.pn2_bn_finalize(_p(stats), P, co, _p(gamma), _p(beta), eps, mom, int(training), _p(rmean), _p(rvar), _p(nbt),
                                   _p(aff), st), "pn2_bn_finalize")
        z = _empty_rows(P, co, dev)
        _check(lib.pn2_bn_relu_max(_p(y), y.shape[1], _p(aff), P, 1, co, _p(z), z.shape[1], None, None, st), "pn2_bn_relu_max")
        if training:
            bump_param_generation()
        ctx.save_for_backward(pf, g, y, z, aff, w, gamma)
        ctx.meta = (N, bool(training), P, B, co, cg, cp, ct)
        return z[:, :co] if z.shape[1] != co else z

    @staticmethod
    def backward(ctx, grad):
        lib, st = _lib.load(), _lib.stream()
        pf, g, y, z, aff, w, gamma = ctx.saved_tensors
        N, training, P, B, co, cg, cp, ct = ctx.meta
        dev = pf.device
        wc = _contig_weight(w)
        ldz = z.shape[1]
        grad = grad.contiguous().float()
        if grad.shape[1] != ldz:
            grad = F.pad(grad, (0, ldz - grad.shape[1]))
        red, coef, dW, db = _carve(dev, [(torch.float64, _REPL * 2 * co), (torch.float32, 4 * _r4(co)), (torch.float32, co * ct),
                                         (torch.float32, co)])
        dW = dW.view(co, ct)
        dZ = _empty_rows(P, co, dev)
        _check(lib.pn2_relu_bwd_reduce(_p(grad), ldz, _p(z), _p(y), y.shape[1], _p(aff), P, co, _p(dZ), dZ.shape[1], _p(red), st),
               "pn2_relu_bwd_reduce")
        dgamma = torch.empty(co, device=dev, dtype=torch.float32)
        dbeta = torch.empty(co, device=dev, dtype=torch.float32)
        _check(lib.pn2_bn_bwd_coef(_p(red), P, co, _p(gamma), _p(aff), int(training), _p(coef), _p(dgamma), _p(dbeta), 0, st),
               "pn2_bn_bwd_coef")
        ldy = y.shape[1]
        # per-point part: dW_p += dY^T pointfeat, d pointfeat = dY W_p  (W_p: columns cg.. of the weight, pitch ct)
        dy = _UpGrad.dense(dZ, y, coef)
        _check(lib.pn2_conv1x1_wgrad(*dy, _p(pf), pf.shape[1], None, dW.data_ptr() + 4 * cg, ct, None, P, co, cp, None, st),
               "pn2_conv1x1_wgrad")
        dpf = None
        if ctx.needs_input_grad[0]:
            dpf = torch.empty(P, pf.shape[1], device=dev, dtype=torch.float32)
            _check(lib.pn2_conv1x1_dgrad(*dy, wc.data_ptr() + 4 * cg, ct, None, 0, None, _p(dpf), dpf.shape[1], None, P, co, cp, None, st),
                   "pn2_conv1x1_dgrad")
        # per-cloud part: s_b = sum_{p in b} dY_p, then [B]-row GEMMs with the identity coefficients (dY := s)
        s = _empty_rows(B, co, dev)
        ws = torch.empty(int(lib.pn2_group_colsum_workspace_bytes(P, N, co)), device=dev, dtype=torch.uint8)
        _check(lib.pn2_group_colsum(_p(dZ), dZ.shape[1], _p(y), ldy, _p(coef), P, N, co, _p(s), s.shape[1], _p(ws), st), "pn2_group_colsum")
        ds = _UpGrad.linear(s, co)
        _check(lib.pn2_conv1x1_wgrad(*ds, _p(g), cg, None, _p(dW), ct, _p(db), B, co, cg, None, st), "pn2_conv1x1_wgrad")
        dg = None
        if ctx.needs_input_grad[1]:
            dg = torch.empty(B, cg, device=dev, dtype=torch.float32)
            _check(lib.pn2_conv1x1_dgrad(*ds, _p(wc), ct, None, 0, None, _p(dg), cg, None, B, co, cg, None, st), "pn2_conv1x1_dgrad")
        return dpf, dg, None, None, None, dW.view_as(w), db, dgamma, dbeta, None, None, None


def global_concat_conv(pointfeat, g, conv, bn, N, training):
    """relu(bn(conv(cat([g.repeat(N), pointfeat])))) on rows: pointfeat [B*N, C_p], g [B, C_g] -> [B*N, C_out] (HIP)."""
    pointfeat = _gpu_f32(pointfeat, "pointfeat")
    g = _gpu_f32(g, "global feature")
    B, cg = g.shape
    if pointfeat.shape[0] != B * N or conv.in_channels != cg + pointfeat.shape[1] or cg % 4 or pointfeat.shape[1] % 4:
        raise RuntimeError("global_concat_conv: shapes do not match the layer")
    return _GlobalConcatConv.apply(pointfeat, g, N, bool(training), _bn_cfg(bn), conv.weight, conv.bias, bn.weight, bn.bias,
                                   bn.running_mean, bn.running_var, bn.num_batches_tracked)


def _stn_from_rows(stn, rows, B, N, k):
    """conv1-3 + BN + ReLU pooled over the whole cloud (HIP), then the fully connected head on [B, 1024] (stock PyTorch)."""
    x = shared_mlp(rows, k, [stn.conv1, stn.conv2, stn.conv3], [stn.bn1, stn.bn2, stn.bn3], N, stn.training)
    x = F.relu(stn.bn4(stn.fc1(x)))
    x = F.relu(stn.bn5(stn.fc2(x)))
    x = stn.fc3(x)
    iden = torch.eye(k, device=x.device, dtype=x.dtype).reshape(1, k * k)
    return (x + iden).view(-1, k, k)


class STN3d(nn.Module):
    """model/pointnet.py STN3d: [B, 3, N] -> [B, 3, 3]."""

    def __init__(self):
        super().__init__()
        self.conv1 = torch.nn.Conv1d(3, 64, 1)
        self.conv2 = torch.nn.Conv1d(64, 128, 1)
        self.conv3 = torch.nn.Conv1d(128, 1024, 1)
        self.fc1 = nn.Linear(1024, 512)
        self.fc2 = nn.Linear(512, 256)
        self.fc3 = nn.Linear(256, 9)
        self.relu = nn.ReLU()

        self.bn1 = nn.BatchNorm1d(64)
        self.bn2 = nn.BatchNorm1d(128)
        self.bn3 = nn.BatchNorm1d(1024)
        self.bn4 = nn.BatchNorm1d(512)
        self.bn5 = nn.BatchNorm1d(256)

    def forward(self, x):
        B, _, N = x.shape
        return _stn_from_rows(self, _rows(x), B, N, 3)


class STNkd(nn.Module):
    """model/pointnet.py STNkd: [B, k, N] -> [B, k, k]."""

    def __init__(self, k=64):
        super().__init__()
        self.conv1 = torch.nn.Conv1d(k, 64, 1)
        self.conv2 = torch.nn.Conv1d(64, 128, 1)
        self.conv3 = torch.nn.Conv1d(128, 1024, 1)
        self.fc1 = nn.Linear(1024, 512)
        self.fc2 = nn.Linear(512, 256)
        self.fc3 = nn.Linear(256, k * k)
        self.relu = nn.ReLU()

        self.bn1 = nn.BatchNorm1d(64)
        self.bn2 = nn.BatchNorm1d(128)
        self.bn3 = nn.BatchNorm1d(1024)
        self.bn4 = nn.BatchNorm1d(512)
        self.bn5 = nn.BatchNorm1d(256)

        self.k = k

    def forward(self, x):
        B, _, N = x.shape
        return _stn_from_rows(self, _rows(x), B, N, self.k)


class PointNetEncoder(nn.Module):
    """model/pointnet.py PointNetEncoder.  As in the reference the input transform is STNkd(k=input_dims), the last layer has
    no ReLU before the max, and with the feature transform ``pointfeat`` is the transformed tensor."""

    def __init__(self, global_feat=True, input_dims=4, feature_transform=False):
        super().__init__()
        self.stn = STNkd(k=input_dims)
        self.conv1 = torch.nn.Conv1d(input_dims, 64, 1)
        self.conv2 = torch.nn.Conv1d(64, 128, 1)
        self.conv3 = torch.nn.Conv1d(128, 1024, 1)
        self.bn1 = nn.BatchNorm1d(64)
        self.bn2 = nn.BatchNorm1d(128)
        self.bn3 = nn.BatchNorm1d(1024)
        self.global_feat = global_feat
        self.feature_transform = feature_transform
        if self.feature_transform:
            self.fstn = STNkd(k=64)

    def features(self, x):
        """x [B, C, N] -> (global feature [B, 1024], pointfeat rows [B*N, 64], trans, trans_feat)."""
        B, C, N = x.shape
        rows = _rows(x)
        trans = _stn_from_rows(self.stn, rows, B, N, C)
        h = shared_mlp(point_transform(rows, trans, B, N, C), C, [self.conv1], [self.bn1], 0, self.training)
        trans_feat = None
        if self.feature_transform:
            trans_feat = _stn_from_rows(self.fstn, h, B, N, 64)
            h = point_transform(h, trans_feat, B, N, 64)
        h2 = shared_mlp(h, 64, [self.conv2], [self.bn2], 0, self.training)
        g = conv_bn_max(h2, self.conv3, self.bn3, N, self.training)
        return g, h, trans, trans_feat

    def forward(self, x):
        B, _, N = x.shape
        g, pointfeat, trans, trans_feat = self.features(x)
        if self.global_feat:
            return g, trans, trans_feat
        # the reference's [B, 1088, N] output for callers of the encoder itself (PointNetSeg never forms it)
        pf = pointfeat.view(B, N, -1).permute(0, 2, 1)
        return torch.cat([g.view(B, -1, 1).expand(B, g.shape[1], N), pf], 1), trans, trans_feat


class PointNetCls(nn.Module):
    """model/pointnet.py PointNetCls (ModelNet40, clf.py): returns (log_probs [B, k], trans_feat)."""

    def __init__(self, k=2, feature_transform=False):
        super().__init__()
        self.feature_transform = feature_transform
        self.feat = PointNetEncoder(global_feat=True, feature_transform=feature_transform, input_dims=3)
        self.fc1 = nn.Linear(1024, 512)
        self.fc2 = nn.Linear(512, 256)
        self.fc3 = nn.Linear(256, k)
        self.dropout = nn.Dropout(p=0.3)
        self.bn1 = nn.BatchNorm1d(512)
        self.bn2 = nn.BatchNorm1d(256)
        self.relu = nn.ReLU()

    def forward(self, x):
        x, trans, trans_feat = self.feat(x)
        x = F.relu(self.bn1(self.fc1(x)))
        x = F.relu(self.bn2(self.dropout(self.fc2(x))))          # (dropout before bn2, as the reference)
        x = self.fc3(x)
        return F.log_softmax(x, dim=1), trans_feat


class PointNetSeg(nn.Module):
    """model/pointnet.py PointNetSeg (semseg.py / pcdseg.py / pcdvis.py): returns (log_probs [B, N, k], trans_feat)."""

    def __init__(self, num_class, input_dims=4, feature_transform=False):
        super().__init__()
        self.k = num_class
        self.feat = PointNetEncoder(global_feat=False, input_dims=input_dims, feature_transform=feature_transform)
        self.conv1 = torch.nn.Conv1d(1088, 512, 1)
        self.conv2 = torch.nn.Conv1d(512, 256, 1)
        self.conv3 = torch.nn.Conv1d(256, 128, 1)
        self.conv4 = torch.nn.Conv1d(128, self.k, 1)
        self.bn1 = nn.BatchNorm1d(512)
        self.bn2 = nn.BatchNorm1d(256)
        self.bn3 = nn.BatchNorm1d(128)

    def forward(self, x):
        B, _, N = x.shape
        g, pointfeat, trans, trans_feat = self.feat.features(x)
        h = global_concat_conv(pointfeat, g, self.conv1, self.bn1, N, self.training)      # concat order [global, pointfeat]
        h = shared_mlp(h, 512, [self.conv2, self.conv3], [self.bn2, self.bn3], 0, self.training)
        logits = conv1x1(h, self.conv4, padded=True)
        return log_softmax_rows(logits, self.k).view(B, N, self.k), trans_feat


class PointNetColorGen(PointNetSeg):
    """data_utils/ColorGenerator_Loader.py:1-24 PointNetColorGen (the colour-generation task: a colour per point): ``PointNetSeg``
    without the log-softmax, returns ``(x [B, N, k], trans_feat)``.  Its ``state_dict`` keys are ``PointNetSeg``'s, so
    ``pointnet2.load_reference_state`` loads a reference checkpoint.  The ``k`` columns are a slice of the padded rows the last GEMM
    wrote (pitch ``round4(k)``): no copy is made, and the tensor is not contiguous unless ``k`` is a multiple of 4."""

    def forward(self, x):
        B, _, N = x.shape
        g, pointfeat, trans, trans_feat = self.feat.features(x)
        h = global_concat_conv(pointfeat, g, self.conv1, self.bn1, N, self.training)
        h = shared_mlp(h, 512, [self.conv2, self.conv3], [self.bn2, self.bn3], 0, self.training)
        return conv1x1(h, self.conv4, padded=True)[:, :self.k].view(B, N, self.k), trans_feat


class _DenseSegHead(torch.autograd.Function):
    """PointNetDenseCls from out4 on: conv5 + bn5 (no ReLU) + max over the cloud -> out_max, and
    relu(bns1(convs1(cat([cat([out_max, label]).repeat(N), out1, out2, out3, out4, out5])))) as rows.

    The [B*N, 4944] concatenation and bn5's per-point output are never built.  convs1 is W_g g_b (one [B]-row GEMM,
    g = [out_max | label]) added in the epilogue of ONE per-point GEMM over the five sources read in place
    (pn2_conv1x1_fwd_multi); out5 is bn5 applied by that GEMM's loader to the saved pre-BN conv5 output.  Backward: convs1's
    weight gradient in one launch over the sources (pn2_conv1x1_wgrad_multi), its per-cloud part from the column sums of dY,
    the data gradients per source (pn2_conv1x1_dgrad_multi); bn5 sees the dense gradient from convs1 plus, at the arg-max rows,
    the pooled gradient from both heads (pn2_bn_bwd_reduce_noact_dense); conv5's data gradient is added to out4's."""

    @staticmethod
    def forward(ctx, o1, o2, o3, o4, label, N, training, cfg5, cfgs1, w5, b5, g5, be5, rm5, rv5, nbt5, ws1, bs1, gs1, bes1, rms1, rvs1,
                nbts1):
        lib, st = _lib.load(), _lib.stream()
        dev = o4.device
        P = o4.shape[0]
        B = P // N
        c5, ci5 = w5.shape[0], w5.shape[1]
        co, ct = ws1.shape[0], ws1.shape[1]
        cg = c5 + label.shape[1]
        srcs = (o1, o2, o3, o4)
        stats5, stats1, aff5, aff1, zero_bias = _carve(dev, [(torch.float64, _REPL * 2 * c5), (torch.float64, _REPL * 2 * co),
                                                             (torch.float32, 4 * _r4(c5)), (torch.float32, 4 * _r4(co)),
                                                             (torch.float32, co)])
        # conv5 + bn5 + max over the cloud (the pre-BN output is kept: bn5 is applied by its consumers)
        y5 = _empty_rows(P, c5, dev)
        _check(lib.pn2_conv1x1_fwd(_p(o4), o4.shape[1], None, _p(_contig_weight(w5)), ci5, _p(b5), _p(y5), y5.shape[1], P, ci5, c5,
                                   _p(stats5) if training else None, None, st), "pn2_conv1x1_fwd")
        eps, mom = cfg5
        _check(lib.pn2_bn_finalize(_p(stats5), P, c5, _p(g5), _p(be5), eps, mom, int(training), _p(rm5), _p(rv5), _p(nbt5), _p(aff5), st),
               "pn2_bn_finalize")
        omax = _empty_rows(B, c5, dev)
        arg = torch.empty(B, omax.shape[1], device=dev, dtype=torch.int32)
        _check(lib.pn2_bn_max(_p(y5), y5.shape[1], _p(aff5), B, N, c5, _p(omax), omax.shape[1], _p(arg), st), "pn2_bn_max")
        # convs1: W_g g_b per cloud, then one GEMM over out1 .. out5 with that term and the statistics in its epilogue
        g = torch.cat([omax[:, :c5], label], 1)
        if cg % 4:
            g = F.pad(g, (0, _r4(cg) - cg))
        wc = _contig_weight(ws1)
        gterm = _empty_rows(B, co, dev)
        _check(lib.pn2_conv1x1_fwd(_p(g), g.shape[1], None, _p(wc), ct, _p(zero_bias), _p(gterm), gterm.shape[1], B, cg, co, None, None,
                                   st), "pn2_conv1x1_fwd")
        table = _lib.src_table([(_p(s), s.shape[1], s.shape[1], None, 0) for s in srcs] + [(_p(y5), y5.shape[1], c5, _p(aff5), 0)])
        y1 = _empty_rows(P, co, dev)
        _check(lib.pn2_conv1x1_fwd_multi(table, len(table), wc.data_ptr() + 4 * cg, ct, _p(bs1), _p(gterm), gterm.shape[1], N, _p(y1),
                                         y1.shape[1], P, co, _p(stats1) if training else None, st), "pn2_conv1x1_fwd_multi")
        eps, mom = cfgs1
        _check(lib.pn2_bn_finalize(_p(stats1), P, co, _p(gs1), _p(bes1), eps, mom, int(training), _p(rms1), _p(rvs1), _p(nbts1), _p(aff1),
                                   st), "pn2_bn_finalize")
        z = _empty_rows(P, co, dev)
        _check(lib.pn2_bn_relu_max(_p(y1), y1.shape[1], _p(aff1), P, 1, co, _p(z), z.shape[1], None, None, st), "pn2_bn_relu_max")
        if training:
            bump_param_generation()             # running statistics were written through raw pointers
        ctx.save_for_backward(o1, o2, o3, o4, g, y5, aff5, arg, y1, z, aff1, w5, g5, ws1, gs1)
        ctx.meta = (N, bool(training), P, B, c5, ci5, co, ct, cg)
        return (omax[:, :c5] if omax.shape[1] != c5 else omax), (z[:, :co] if z.shape[1] != co else z)

    @staticmethod
    def backward(ctx, g_max, g_seg):
        lib, st = _lib.load(), _lib.stream()
        o1, o2, o3, o4, g, y5, aff5, arg, y1, z, aff1, w5, g5, ws1, gs1 = ctx.saved_tensors
        N, training, P, B, c5, ci5, co, ct, cg = ctx.meta
        dev = o4.device
        srcs = (o1, o2, o3, o4)
        ld1, ld5 = y1.shape[1], y5.shape[1]
        g_seg = g_seg.contiguous().float()
        if g_seg.shape[1] != ld1:
            g_seg = F.pad(g_seg, (0, ld1 - g_seg.shape[1]))
        red1, red5, coef1, coef5, dW1, db1, dW5, db5 = _carve(dev, [
            (torch.float64, _REPL * 2 * co), (torch.float64, _REPL * 2 * c5), (torch.float32, 4 * _r4(co)), (torch.float32, 4 * _r4(c5)),
            (torch.float32, co * ct), (torch.float32, co), (torch.float32, c5 * ci5), (torch.float32, c5)])
        dW1, dW5 = dW1.view(co, ct), dW5.view(c5, ci5)
        # bns1 + ReLU backward
        dZ1 = _empty_rows(P, co, dev)
        _check(lib.pn2_relu_bwd_reduce(_p(g_seg), ld1, _p(z), _p(y1), ld1, _p(aff1), P, co, _p(dZ1), dZ1.shape[1], _p(red1), st),
               "pn2_relu_bwd_reduce")
        dgs1 = torch.empty(co, device=dev, dtype=torch.float32)
        dbes1 = torch.empty(co, device=dev, dtype=torch.float32)
        _check(lib.pn2_bn_bwd_coef(_p(red1), P, co, _p(gs1), _p(aff1), int(training), _p(coef1), _p(dgs1), _p(dbes1), 0, st),
               "pn2_bn_bwd_coef")
        table = _lib.src_table([(_p(s), s.shape[1], s.shape[1], None, 0) for s in srcs] + [(_p(y5), ld5, c5, _p(aff5), 0)])
        wc = _contig_weight(ws1)
        # convs1, per-point part: one weight-gradient launch over the five sources, data gradients per source
        _check(lib.pn2_conv1x1_wgrad_multi(_p(dZ1), dZ1.shape[1], _p(y1), ld1, _p(coef1), table, len(table), dW1.data_ptr() + 4 * cg, ct, None,
                                           P, co, st), "pn2_conv1x1_wgrad_multi")
        dsrc = [torch.empty(P, s.shape[1], device=dev, dtype=torch.float32) for s in srcs] + [_empty_rows(P, c5, dev)]
        ptrs = (ctypes.c_void_p * 5)(*[_p(d) for d in dsrc])
        lds = (ctypes.c_int * 5)(*[d.shape[1] for d in dsrc])
        ks = (ctypes.c_int * 5)(*([s.shape[1] for s in srcs] + [c5]))
        _check(lib.pn2_conv1x1_dgrad_multi(_p(dZ1), dZ1.shape[1], _p(y1), ld1, _p(coef1), wc.data_ptr() + 4 * cg, ct, ptrs, lds, ks, 5, P, co,
                                           st), "pn2_conv1x1_dgrad_multi")
        # convs1, per-cloud part: s_b = sum_{p in b} dY_p; dW_g += s^T g, db = sum_b s_b, dg = s W_g
        s = _empty_rows(B, co, dev)
        ws = torch.empty(int(lib.pn2_group_colsum_workspace_bytes(P, N, co)), device=dev, dtype=torch.uint8)
        _check(lib.pn2_group_colsum(_p(dZ1), dZ1.shape[1], _p(y1), ld1, _p(coef1), P, N, co, _p(s), s.shape[1], _p(ws), st),
               "pn2_group_colsum")
        ds = _UpGrad.linear(s, co)
        _check(lib.pn2_conv1x1_wgrad(*ds, _p(g), g.shape[1], None, _p(dW1), ct, _p(db1), B, co, cg, None, st), "pn2_conv1x1_wgrad")
        dg = torch.empty(B, g.shape[1], device=dev, dtype=torch.float32)
        _check(lib.pn2_conv1x1_dgrad(*ds, _p(wc), ct, None, 0, None, _p(dg), dg.shape[1], None, B, co, cg, None, st), "pn2_conv1x1_dgrad")
        # bn5: the dense gradient from convs1 plus the pooled one (classification head + per-cloud part of convs1) at the arg-max rows
        dpool = dg[:, :c5]
        if g_max is not None:
            dpool = dpool + g_max.float()
        dpool = dpool.contiguous()
        if dpool.shape[1] != ld5:
            dpool = F.pad(dpool, (0, ld5 - dpool.shape[1]))
        d5 = dsrc[4]
        _check(lib.pn2_bn_bwd_reduce_noact_dense(_p(d5), ld5, _p(dpool), dpool.shape[1], _p(arg), arg.shape[1], _p(y5), ld5, _p(aff5), B, N,
                                                 c5, _p(d5), ld5, _p(red5), st), "pn2_bn_bwd_reduce_noact_dense")
        dg5 = torch.empty(c5, device=dev, dtype=torch.float32)
        dbe5 = torch.empty(c5, device=dev, dtype=torch.float32)
        _check(lib.pn2_bn_bwd_coef(_p(red5), P, c5, _p(g5), _p(aff5), int(training), _p(coef5), _p(dg5), _p(dbe5), 0, st), "pn2_bn_bwd_coef")
        dy5 = _UpGrad.dense(d5, y5, coef5)
        _check(lib.pn2_conv1x1_wgrad(*dy5, _p(o4), o4.shape[1], None, _p(dW5), ci5, None if training else _p(db5), P, c5, ci5, None, st),
               "pn2_conv1x1_wgrad")
        d4 = torch.empty(P, o4.shape[1], device=dev, dtype=torch.float32)
        _check(lib.pn2_conv1x1_dgrad(*dy5, _p(_contig_weight(w5)), ci5, None, 0, None, _p(d4), d4.shape[1], None, P, c5, ci5, None, st),
               "pn2_conv1x1_dgrad")
        d4 += dsrc[3]
        dlabel = dg[:, c5:cg] if ctx.needs_input_grad[4] else None
        return (dsrc[0], dsrc[1], dsrc[2], d4, dlabel, None, None, None, None, dW5.view_as(w5), db5, dg5, dbe5, None, None, None,
                dW1.view_as(ws1), db1, dgs1, dbes1, None, None, None)


def dense_seg_head(out1, out2, out3, out4, label, net, N, training):
    """(out_max [B, 2048], relu(bns1(convs1(concat))) rows [B*N, 256]) of a PointNetDenseCls ``net`` (HIP)."""
    rows = [_gpu_f32(t, "rows") for t in (out1, out2, out3, out4)]
    label = _gpu_f32(label, "label")
    for r, conv in zip(rows, (net.conv1, net.conv2, net.conv3, net.conv4)):
        if r.shape != (rows[0].shape[0], conv.out_channels) or conv.out_channels % 4:
            raise RuntimeError("dense_seg_head: rows must be [B*N, C_out] of conv1 .. conv4")
    if rows[0].shape[0] % N or label.shape[0] != rows[0].shape[0] // N:
        raise RuntimeError("dense_seg_head: label must be [B, cat_num]")
    return _DenseSegHead.apply(rows[0], rows[1], rows[2], rows[3], label, N, bool(training), _bn_cfg(net.bn5), _bn_cfg(net.bns1),
                               net.conv5.weight, net.conv5.bias, net.bn5.weight, net.bn5.bias, net.bn5.running_mean, net.bn5.running_var,
                               net.bn5.num_batches_tracked, net.convs1.weight, net.convs1.bias, net.bns1.weight, net.bns1.bias,
                               net.bns1.running_mean, net.bns1.running_var, net.bns1.num_batches_tracked)


class PointNetDenseCls(nn.Module):
    """model/pointnet.py PointNetDenseCls (ShapeNet part segmentation, partseg.py): forward(point_cloud [B, 3, N], label [B, cat_num]
    one-hot float) returns (net [B, cat_num], net2 [B, N, part_num], trans_feat [B, 128, 128]).

    The reference's quirks are kept: ``net`` is raw logits (not log-softmaxed; PointNetLoss applies nll_loss to them as they are);
    the classification head applies dropout BEFORE bnc2; ``out3`` in the concatenation is the UN-transformed
    relu(bn3(conv3(.))) -- the feature transform feeds conv4 only; ``out5`` is bn5(conv5(.)) without a ReLU, and the max and convs1
    both see that same value.  convs1 takes 4944 channels, which is 2048 + cat_num + 2880 only for cat_num = 16: with any other
    cat_num the reference constructs the network but its forward fails, and so does this one (with a RuntimeError saying why).

    Per-point work runs on the HIP library: shared_mlp for conv1 .. conv4 (one layer per call, so that each output is a convs1
    source), point_transform for both transforms, and conv5 .. convs1 in dense_seg_head (csrc/pointnet_dense.hip, mlp.hip).  The
    [B, .] classification head stays stock PyTorch, as in PointNetCls."""

    def __init__(self, cat_num=16, part_num=50):
        super().__init__()
        self.cat_num = cat_num
        self.part_num = part_num
        self.stn = STN3d()
        self.conv1 = torch.nn.Conv1d(3, 64, 1)
        self.conv2 = torch.nn.Conv1d(64, 128, 1)
        self.conv3 = torch.nn.Conv1d(128, 128, 1)
        self.conv4 = torch.nn.Conv1d(128, 512, 1)
        self.conv5 = torch.nn.Conv1d(512, 2048, 1)
        self.bn1 = nn.BatchNorm1d(64)
        self.bn2 = nn.BatchNorm1d(128)
        self.bn3 = nn.BatchNorm1d(128)
        self.bn4 = nn.BatchNorm1d(512)
        self.bn5 = nn.BatchNorm1d(2048)
        self.fstn = STNkd(k=128)
        # classification network
        self.fc1 = nn.Linear(2048, 256)
        self.fc2 = nn.Linear(256, 256)
        self.fc3 = nn.Linear(256, cat_num)
        self.dropout = nn.Dropout(p=0.3)
        self.bnc1 = nn.BatchNorm1d(256)
        self.bnc2 = nn.BatchNorm1d(256)
        # segmentation network
        self.convs1 = torch.nn.Conv1d(4944, 256, 1)
        self.convs2 = torch.nn.Conv1d(256, 256, 1)
        self.convs3 = torch.nn.Conv1d(256, 128, 1)
        self.convs4 = torch.nn.Conv1d(128, part_num, 1)
        self.bns1 = nn.BatchNorm1d(256)
        self.bns2 = nn.BatchNorm1d(256)
        self.bns3 = nn.BatchNorm1d(128)

    def forward(self, point_cloud, label):
        B, C, N = point_cloud.shape
        if C != 3:
            raise RuntimeError("PointNetDenseCls: point_cloud must be [B, 3, N]")
        if label.dim() != 2 or label.shape[0] != B or 2048 + label.shape[1] + 2880 != self.convs1.in_channels:
            raise RuntimeError("PointNetDenseCls: label must be [B, %d] (convs1 takes %d = 2048 + cat_num + 2880 channels)"
                               % (self.convs1.in_channels - 4928, self.convs1.in_channels))
        rows = _rows(point_cloud)
        trans = _stn_from_rows(self.stn, rows, B, N, 3)
        h = point_transform(rows, trans, B, N, 3)
        out1 = shared_mlp(h, 3, [self.conv1], [self.bn1], 0, self.training)
        out2 = shared_mlp(out1, 64, [self.conv2], [self.bn2], 0, self.training)
        out3 = shared_mlp(out2, 128, [self.conv3], [self.bn3], 0, self.training)
        trans_feat = _stn_from_rows(self.fstn, out3, B, N, 128)
        out4 = shared_mlp(point_transform(out3, trans_feat, B, N, 128), 128, [self.conv4], [self.bn4], 0, self.training)
        out_max, h = dense_seg_head(out1, out2, out3, out4, label, self, N, self.training)
        # classification network ([B, .]: stock PyTorch; dropout before bnc2, no log_softmax -- as the reference)
        net = F.relu(self.bnc1(self.fc1(out_max)))
        net = F.relu(self.bnc2(self.dropout(self.fc2(net))))
        net = self.fc3(net)
        # segmentation network
        h = shared_mlp(h, 256, [self.convs2, self.convs3], [self.bns2, self.bns3], 0, self.training)
        logits = conv1x1(h, self.convs4, padded=True)
        return net, log_softmax_rows(logits, self.part_num).view(B, N, self.part_num), trans_feat


class PointNetLoss(torch.nn.Module):
    """model/pointnet.py PointNetLoss: (loss, seg_loss, label_loss) with
    loss = weight * seg_loss + (1 - weight) * label_loss + mat_diff_loss_scale * feature_transform_reguliarzer(trans_feat), where
    seg_loss = nll_loss(seg_pred, seg) and label_loss = nll_loss(labels_pred, label) on the RAW logits of PointNetDenseCls's
    ``net``, exactly as the reference computes it.  seg_loss of GPU tensors runs on the HIP library (pointnet12_amd.loss)."""

    def __init__(self, weight=1, mat_diff_loss_scale=0.001):
        super().__init__()
        self.mat_diff_loss_scale = mat_diff_loss_scale
        self.weight = weight

    def forward(self, labels_pred, label, seg_pred, seg, trans_feat):
        seg_loss = nll_loss(seg_pred, seg) if seg_pred.is_cuda else F.nll_loss(seg_pred, seg)
        mat_diff_loss = feature_transform_reguliarzer(trans_feat)
        label_loss = F.nll_loss(labels_pred, label)
        loss = self.weight * seg_loss + (1 - self.weight) * label_loss + mat_diff_loss * self.mat_diff_loss_scale
        return loss, seg_loss, label_loss


def feature_transform_reguliarzer(trans):
    """mean_b || T_b (T_b^T - I) ||_F, exactly as the reference writes it (not T T^T - I).  Stock PyTorch on [B, k, k]."""
    d = trans.size()[1]
    eye = torch.eye(d, device=trans.device, dtype=trans.dtype)[None, :, :]
    return torch.mean(torch.norm(torch.bmm(trans, trans.transpose(2, 1) - eye), dim=(1, 2)))


feature_transform_regularizer = feature_transform_reguliarzer       # the correct spelling
