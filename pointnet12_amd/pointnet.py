"""MI355X-native counterpart of the reference's ``model/pointnet.py`` (PointNet v1).

Same class names, constructor arguments, attribute names and registration order as the reference (``STN3d``, ``STNkd``,
``PointNetEncoder``, ``PointNetCls``, ``PointNetSeg``, ``feature_transform_reguliarzer``), so ``state_dict`` keys, shapes and
seeded initial values are the reference's and its checkpoints load with ``pointnet2.load_reference_state``.

Every per-point operation runs on the HIP library: the conv + BatchNorm + ReLU stacks (the STN stacks pooled over the whole
cloud included) through ``shared_mlp``, ``torch.bmm(x, trans)`` through ``pn2_point_transform``, the encoder's conv3 + bn3 + max
(no ReLU) through ``pn2_bn_max``, and the segmentation head's conv1 over ``cat([global.repeat(N), pointfeat])`` factorised as
``W_p pointfeat_p + b + W_g g_b`` -- the [B*N, 1088] concatenation never exists.  Work on [B, .] vectors (the STN fully
connected layers, the classification head, the regulariser) stays stock PyTorch, as the PointNet++ classification head does.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import check as _check, ptr as _p
from .pointnet_util import (_REPL, _channel_last, _contig_weight, _empty_rows, _gpu_f32, _ident_coef, _r4, _zeros_small,
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
        zb = _zeros_small(8 * _REPL * 2 * co + 16 * _r4(co), dev)
        stats = zb[:8 * _REPL * 2 * co].view(torch.float64)
        aff = zb[8 * _REPL * 2 * co:].view(torch.float32)
        y = _empty_rows(P, co, dev)
        _check(lib.pn2_conv1x1_fwd(_p(x), ldx, None, _p(_contig_weight(w)), ci, _p(b), _p(y), y.shape[1], P, ci, co,
                                   _p(stats) if training else None, None, None, st), "pn2_conv1x1_fwd")
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
        if grad.stride(-1) != 1 or grad.dtype != torch.float32:
            grad = grad.contiguous().float()
        zb = _zeros_small(8 * _REPL * 2 * co + 16 * _r4(co) + 4 * (co * ci + co), dev)
        red = zb[:8 * _REPL * 2 * co].view(torch.float64)
        rest = zb[8 * _REPL * 2 * co:].view(torch.float32)
        coef = rest[:4 * _r4(co)]
        dW = rest[4 * _r4(co):4 * _r4(co) + co * ci].view(co, ci)
        db = rest[4 * _r4(co) + co * ci:]
        dzp = torch.empty(G, ldo, device=dev, dtype=torch.float32)
        _check(lib.pn2_pool_bwd_reduce_noact(_p(grad), grad.stride(0), _p(arg), ldo, _p(y), y.shape[1], _p(aff), G, N, co, _p(dzp),
                                             _p(red), st), "pn2_pool_bwd_reduce_noact")
        dgamma = torch.empty(co, device=dev, dtype=torch.float32)
        dbeta = torch.empty(co, device=dev, dtype=torch.float32)
        _check(lib.pn2_bn_bwd_coef(_p(red), P, co, _p(gamma), _p(aff), int(training), _p(coef), _p(dgamma), _p(dbeta), 0, st),
               "pn2_bn_bwd_coef")
        _check(lib.pn2_conv1x1_wgrad(None, 0, _p(dzp), ldo, _p(arg), N, _p(y), y.shape[1], _p(coef), _p(x), x.shape[1], None, _p(dW), ci,
                                     None if training else _p(db), P, co, ci, None, st), "pn2_conv1x1_wgrad")
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(P, x.shape[1], device=dev, dtype=torch.float32)
            _check(lib.pn2_conv1x1_dgrad(None, 0, _p(dzp), ldo, _p(arg), N, _p(y), y.shape[1], _p(coef), _p(_contig_weight(w)), ci,
                                         None, 0, None, _p(dx), dx.shape[1], None, P, co, ci, None, None, st), "pn2_conv1x1_dgrad")
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
        zb = _zeros_small(8 * _REPL * 2 * co + 16 * _r4(co) + 4 * co, dev)
        stats = zb[:8 * _REPL * 2 * co].view(torch.float64)
        aff = zb[8 * _REPL * 2 * co:8 * _REPL * 2 * co + 16 * _r4(co)].view(torch.float32)
        zero_bias = zb[8 * _REPL * 2 * co + 16 * _r4(co):].view(torch.float32)
        gterm = _empty_rows(B, co, dev)                # W_g g_b: one row per cloud
        _check(lib.pn2_conv1x1_fwd(_p(g), cg, None, _p(wc), ct, _p(zero_bias), _p(gterm), gterm.shape[1], B, cg, co, None, None, None, st),
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
        zb = _zeros_small(8 * _REPL * 2 * co + 16 * _r4(co) + 4 * (co * ct + co), dev)
        red = zb[:8 * _REPL * 2 * co].view(torch.float64)
        rest = zb[8 * _REPL * 2 * co:].view(torch.float32)
        coef = rest[:4 * _r4(co)]
        dW = rest[4 * _r4(co):4 * _r4(co) + co * ct].view(co, ct)
        db = rest[4 * _r4(co) + co * ct:]
        dZ = _empty_rows(P, co, dev)
        _check(lib.pn2_relu_bwd_reduce(_p(grad), ldz, _p(z), _p(y), y.shape[1], _p(aff), P, co, _p(dZ), dZ.shape[1], _p(red), None, st),
               "pn2_relu_bwd_reduce")
        dgamma = torch.empty(co, device=dev, dtype=torch.float32)
        dbeta = torch.empty(co, device=dev, dtype=torch.float32)
        _check(lib.pn2_bn_bwd_coef(_p(red), P, co, _p(gamma), _p(aff), int(training), _p(coef), _p(dgamma), _p(dbeta), 0, st),
               "pn2_bn_bwd_coef")
        ldy = y.shape[1]
        # per-point part: dW_p += dY^T pointfeat, d pointfeat = dY W_p  (W_p: columns cg.. of the weight, pitch ct)
        _check(lib.pn2_conv1x1_wgrad(_p(dZ), dZ.shape[1], None, 0, None, 0, _p(y), ldy, _p(coef), _p(pf), pf.shape[1], None,
                                     dW.data_ptr() + 4 * cg, ct, None, P, co, cp, None, st), "pn2_conv1x1_wgrad")
        dpf = None
        if ctx.needs_input_grad[0]:
            dpf = torch.empty(P, pf.shape[1], device=dev, dtype=torch.float32)
            _check(lib.pn2_conv1x1_dgrad(_p(dZ), dZ.shape[1], None, 0, None, 0, _p(y), ldy, _p(coef), wc.data_ptr() + 4 * cg, ct, None, 0,
                                         None, _p(dpf), dpf.shape[1], None, P, co, cp, None, None, st), "pn2_conv1x1_dgrad")
        # per-cloud part: s_b = sum_{p in b} dY_p, then [B]-row GEMMs with the identity coefficients (dY := s)
        s = _empty_rows(B, co, dev)
        ws = torch.empty(int(lib.pn2_group_colsum_workspace_bytes(P, N, co)), device=dev, dtype=torch.uint8)
        _check(lib.pn2_group_colsum(_p(dZ), dZ.shape[1], _p(y), ldy, _p(coef), P, N, co, _p(s), s.shape[1], _p(ws), st), "pn2_group_colsum")
        ident = _ident_coef(co, dev)
        _check(lib.pn2_conv1x1_wgrad(_p(s), s.shape[1], None, 0, None, 0, _p(s), s.shape[1], _p(ident), _p(g), cg, None, _p(dW), ct,
                                     _p(db), B, co, cg, None, st), "pn2_conv1x1_wgrad")
        dg = None
        if ctx.needs_input_grad[1]:
            dg = torch.empty(B, cg, device=dev, dtype=torch.float32)
            _check(lib.pn2_conv1x1_dgrad(_p(s), s.shape[1], None, 0, None, 0, _p(s), s.shape[1], _p(ident), _p(wc), ct, None, 0, None,
                                         _p(dg), cg, None, B, co, cg, None, None, st), "pn2_conv1x1_dgrad")
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


def feature_transform_reguliarzer(trans):
    """mean_b || T_b (T_b^T - I) ||_F, exactly as the reference writes it (not T T^T - I).  Stock PyTorch on [B, k, k]."""
    d = trans.size()[1]
    eye = torch.eye(d, device=trans.device, dtype=trans.dtype)[None, :, :]
    return torch.mean(torch.norm(torch.bmm(trans, trans.transpose(2, 1) - eye), dim=(1, 2)))


feature_transform_regularizer = feature_transform_reguliarzer       # the correct spelling
