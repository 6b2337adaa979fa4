"""Fixed operands and fp64 statements of the conv1x1 entry points (csrc/mlp.hip, mlp_res.hip, mlp_wide.hip): pn2_conv1x1_fwd,
pn2_conv1x1_dgrad / _wgrad, the fused pn2_conv1x1_bwd, and the two BatchNorm blocks they consume (pn2_bn_finalize's affine
block, pn2_bn_bwd_coef's coefficient block).  A test helper written from the formulas of include/pn2.h, for clarity, not
speed; every function takes tensors of any device and answers on that device.

NO DECISION IN THE PATH.  The operands are drawn directly (the pre-BN tensors, the blocks, dZ): the ReLU mask of a case is
that of the given previous output on both sides, the pooled rows are those of the given arg, so no rounding can flip
anything and a result is held to ~1e-6 of its largest entry.

SEAM-SENSITIVE INPUTS (``tail_from``).  The entry points run a leading block of whole tiles in one kernel family and the
ragged remainder in the streamed kernels.  In a case with ``tail_from = r`` the rows >= r of the layer input (X / prev_Y)
and of dZ (pooled: the groups from row r on) are SCALED BY 32: one such row carries 32 x the weight of a leading row in
sum y and in the reductions, and 1024 x in sum y^2 and dW, so a tail row that is dropped or counted twice moves every
column sum by far more than any bound here (one of 131 072 unit rows would move sum y^2 by 8e-6 -- inside 1e-5).

GUARDS.  ``guarded`` allocates an output with GUARD_ROWS extra rows (and whatever extra columns the pitch has) pre-filled
with the bit pattern SENTINEL (a NaN); ``check_guards`` requires rows >= P and columns >= round4(C) to hold it still, every
element inside to have been written, and the pad columns [C, round4(C)) to be zero where include/pn2.h says they are
written: an overrunning whole-tile store is caught inside the allocation, without a fault.
"""
import torch

GUARD_ROWS = 64
SENTINEL = 0x7FA5A5A5                # a NaN: never the bits of a correct result
TAIL_SCALE = 32.0
STAT_REPLICAS = 8                    # PN2_STAT_REPLICAS of include/pn2.h


def round4(c):
    return (c + 3) & ~3


def rel(a, b):
    """Largest difference relative to the reference's largest entry."""
    return float((a.double() - b).abs().max()) / max(float(b.abs().max()), 1e-30)


# ------------------------------------------------------------------------------------------------ guards

def guarded(P, ld, dev):
    """float32 [P + GUARD_ROWS, ld], every element SENTINEL."""
    return torch.full((P + GUARD_ROWS, ld), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)


def check_guards(buf, P, C, what, pad_zero=True):
    bits = buf.view(torch.int32)
    C4 = round4(C)
    assert bool((bits[P:] == SENTINEL).all()), "%s: a row >= %d was written" % (what, P)
    assert bool((bits[:P, C4:] == SENTINEL).all()), "%s: a column >= %d was written" % (what, C4)
    assert not bool((bits[:P, :C] == SENTINEL).any()), "%s: an element of the result was not written" % what
    if pad_zero:
        assert bool((buf[:P, C:C4] == 0).all()), "%s: pad columns [%d, %d) are not zero" % (what, C, C4)


def framed(rows, cols, ld, rnd):
    """An accumulated output (dW, dbias as one row) inside a frame: [rows + 2, ld] random values, the result region
    [:rows, :cols].  Returns (buffer, its initial copy)."""
    buf = rnd(rows + 2, ld)
    return buf, buf.clone()


def check_frame(buf, buf0, rows, cols, what):
    assert torch.equal(buf[rows:], buf0[rows:]) and torch.equal(buf[:rows, cols:], buf0[:rows, cols:]), "%s: written outside [%d, %d]" % (what, rows, cols)


# ------------------------------------------------------------------------------------------------ the two BatchNorm blocks

def affine_block(s1, s2, P, gamma, beta, eps):
    """fp64 [4, C] = [mean | gamma * invstd | beta | invstd] from the per-channel sums of y and y^2 over P rows
    (training-mode BatchNorm: biased variance) -- what pn2_bn_finalize writes at pitch round4(C)."""
    mean = s1.double() / P
    var = torch.clamp(s2.double() / P - mean * mean, min=0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    return torch.stack([mean, gamma.double() * invstd, beta.double(), invstd])


def running_stats(s1, s2, P, momentum, rmean0, rvar0):
    """fp64 running mean / variance after one training step (unbiased variance)."""
    mean = s1.double() / P
    var = torch.clamp(s2.double() / P - mean * mean, min=0.0) * (P / (P - 1.0) if P > 1 else 1.0)
    return (1.0 - momentum) * rmean0.double() + momentum * mean, (1.0 - momentum) * rvar0.double() + momentum * var


def coef_block(r0, r1, P, gamma, mean, invstd):
    """fp64 [4, C] = [c0 | q1 | q0 | mean] from the reductions r0 = sum dZ, r1 = sum dZ * yhat (yhat = (y - mean) * invstd),
    as bn_coef_channel (csrc/bn_affine.h) forms them: c0 = gamma * invstd, q1 = -c0 * invstd * r1 / P, q0 = -c0 * r0 / P."""
    c0 = gamma.double() * invstd.double()
    return torch.stack([c0, -c0 * invstd.double() * r1.double() / P, -c0 * r0.double() / P, mean.double()])


def dy_of(coef, D, Y):
    """dY = c0 dZ + q1 (y - mean) + q0: the gradient with respect to the pre-BN output, from the gradient D with respect to
    the BatchNorm output (already masked by the ReLU) and the coefficient rows [c0 | q1 | q0 | mean]."""
    c0, q1, q0, mu = coef
    return c0 * D + q1 * (Y - mu) + q0


def bn_relu(Yp, aff):
    """The activation the kernels stage from a pre-BN tensor and its affine rows [mean | scale | beta | invstd]: z =
    fma(y - mean, scale, beta) on the fp32-rounded difference (exact in fp64), relu(z) rounded to fp32.  Returns (X, z)."""
    mean, scale, beta = aff[0], aff[1], aff[2]
    z = (Yp - mean).double() * scale.double() + beta.double()
    return torch.clamp(z, min=0).float().double(), z


def replicate(total):
    """[.., C] fp64 column sums -> the PN2_STAT_REPLICAS interleaved copies a producing launch leaves behind (uneven
    shares that add up to `total` in the order the consumers add them)."""
    share = torch.tensor([0.25, 0.0, 0.125, 0.125, 0.0, 0.25, 0.125, 0.125], dtype=torch.float64, device=total.device)
    return (share.view(-1, *([1] * total.dim())) * total.unsqueeze(0)).contiguous()


# ------------------------------------------------------------------------------------------------ operand pieces

def _rnd(dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return g, (lambda *s_: torch.randn(*s_, device=dev, generator=g))


def draw_affine(rnd, C, ld, dev):
    """An affine block [mean | scale | beta | invstd] at pitch ld, pad entries zero."""
    aff = torch.zeros(4 * ld, device=dev)
    aff[:C] = rnd(C) * 0.2
    aff[ld:ld + C] = (rnd(C) * 0.5).abs() + 0.3
    aff[2 * ld:2 * ld + C] = rnd(C) * 0.3
    aff[3 * ld:3 * ld + C] = (rnd(C) * 0.2).abs() + 0.8
    return aff


def draw_coef(rnd, C, ld, dev):
    """A coefficient block [c0 | q1 | q0 | mean] at pitch ld, pad entries zero."""
    coef = torch.zeros(4 * ld, device=dev)
    coef[:C] = rnd(C) * 0.5 + 1.0
    coef[ld:ld + C] = rnd(C) * 1e-3
    coef[2 * ld:2 * ld + C] = rnd(C) * 1e-3
    coef[3 * ld:3 * ld + C] = rnd(C) * 0.3
    return coef


def _draw_weight(rnd, co, ci, mode, dev):
    """W [co, ci] * 0.2 as (view, ldw, storage).  "plain": contiguous.  "slice": columns [3, 3 + ci) of a [co, ci + 3] matrix --
    4-byte offset rows, the guarded scalar loads of BMat; the three leading columns hold large values nobody may read.
    "padded": a 16-byte aligned [co, round4(ci)] copy with zero pad entries -- the float4 loads of BMat."""
    if mode == "plain":
        W = rnd(co, ci) * 0.2
        return W, ci, W
    if mode == "slice":
        store = rnd(co, ci + 3) * 0.2
        store[:, :3] = 1e30
        return store[:, 3:], ci + 3, store
    assert mode == "padded"
    store = torch.zeros(co, round4(ci), device=dev)
    store[:, :ci] = rnd(co, ci) * 0.2
    return store[:, :ci], round4(ci), store


def _rows(P, C, ld, values, poison=1e30):
    """[P, ld] with `values` in the leading C columns, zero pad columns up to round4(C) and, where the pitch is wider,
    large finite values behind them (the columns of a neighbour in a wider matrix: nobody may read them)."""
    t = torch.zeros(P, ld, device=values.device)
    t[:, :C] = values
    t[:, round4(C):] = poison
    return t


# ------------------------------------------------------------------------------------------------ forward

def fixed_forward_case(dev, P, K, N, seed, affine=True, ldx=None, ldy=None, w_mode="plain", tail_from=None):
    """Fixed operands of ONE pn2_conv1x1_fwd call -- X [P, ldx] (a pre-BN tensor with its affine block when `affine`, plain
    rows otherwise), W [N, K] (see _draw_weight), bias -- and the fp64 statement Y = act(X) W^T + b with the per-channel
    sum y, sum y^2 (and sum |y|, the scale the sums' tolerance is relative to).  ldx / ldy default to round4(K) / round4(N);
    rows >= tail_from of X are scaled by TAIL_SCALE (module docstring)."""
    g, rnd = _rnd(dev, seed)
    ldx, ldy = ldx or round4(K), ldy or round4(N)
    xv = rnd(P, K) * 1.5 + 0.3
    if tail_from is not None:
        xv[tail_from:] *= TAIL_SCALE
    X = _rows(P, K, ldx, xv)
    aff = draw_affine(rnd, K, ldx, dev) if affine else None       # (pn2_conv1x1_fwd reads the block at pitch ldx)
    W, ldw, w_store = _draw_weight(rnd, N, K, w_mode, dev)
    bias = rnd(N) * 0.1
    act = bn_relu(X[:, :K], aff.view(4, ldx)[:, :K])[0] if affine else X[:, :K].double()
    Yr = act @ W.double().t() + bias.double()
    ref = {"Y": Yr, "s1": Yr.sum(0), "s2": (Yr * Yr).sum(0), "sabs": Yr.abs().sum(0)}
    return dict(X=X, ldx=ldx, aff=aff, W=W, ldw=ldw, w_store=w_store, bias=bias, ldy=ldy), ref


# ------------------------------------------------------------------------------------------------ backward

def fixed_layer_case(dev, P, co, ci, Kp, seed, masked=True, ldc=None, ldp=None, w_mode="plain", tail_from=None, coef=None):
    """Fixed operands of ONE layer's backward with no decision in the path that rounding could flip: dZ (dense, or the pooled
    pair), Y, the coefficient block, the weight, the previous layer's pre-BN output and affine block -- and the fp64 statement
    of dY = c0 dZ + q1 (y - mean) + q0, dX = (dY W) o mask, dW = dY^T X, db = sum dY, the two reductions of the masked dX.
    masked = False: the layer input is prev_Y as stored (no affine block, no mask, no reductions).  ldc: pitch of dZ / dZp /
    arg / Y (the coefficient block stays at round4(co)); ldp: pitch of prev_Y; both default to round4.  Rows >= tail_from of
    prev_Y and of dZ (pooled: the groups from that row on) are scaled by TAIL_SCALE (module docstring).  coef: a block to use
    instead of the drawn one.  ref["part"](lo, hi) states the column sums (dW, db, r0, r1) over the rows [lo, hi) alone."""
    g, rnd = _rnd(dev, seed)
    c4, p4 = round4(co), round4(ci)
    ldc, ldp = ldc or c4, ldp or p4
    Y = _rows(P, co, ldc, rnd(P, co))
    ypv = rnd(P, ci) * 1.5 + 0.3
    if tail_from is not None:
        ypv[tail_from:] *= TAIL_SCALE
    Yp = _rows(P, ci, ldp, ypv)
    affp = draw_affine(rnd, ci, p4, dev)
    W, ldw, w_store = _draw_weight(rnd, co, ci, w_mode, dev)
    drawn = draw_coef(rnd, co, c4, dev)
    coef = drawn if coef is None else coef
    if Kp:
        G = P // Kp
        dzv = rnd(G, co)
        if tail_from is not None:
            dzv[tail_from // Kp:] *= TAIL_SCALE
        dzp = _rows(G, co, ldc, dzv)
        arg = torch.randint(0, Kp, (G, ldc), device=dev, dtype=torch.int32, generator=g)
        D = torch.zeros(G, Kp, co, device=dev, dtype=torch.float64)
        D.scatter_(1, arg[:, :co].long().unsqueeze(1), dzp[:, :co].double().unsqueeze(1))
        D = D.view(P, co)
        dz_args = (None, 0, dzp.data_ptr(), ldc, arg.data_ptr(), Kp)
        keep = (dzp, arg)
    else:
        dzv = rnd(P, co)
        if tail_from is not None:
            dzv[tail_from:] *= TAIL_SCALE
        dZ = _rows(P, co, ldc, dzv)
        D = dZ[:, :co].double()
        dz_args = (dZ.data_ptr(), ldc, None, 0, None, 0)
        keep = (dZ,)
    ap = affp.view(4, p4)[:, :ci]
    dY = dy_of(coef.view(4, c4)[:, :co].double(), D, Y[:, :co].double())
    if masked:
        X, z = bn_relu(Yp[:, :ci], ap)
        dX = (dY @ W.double()) * (z > 0)
        xhat = (Yp[:, :ci] - ap[0]).double() * ap[3].double()
    else:
        affp, X, xhat = None, Yp[:, :ci].double(), None
        dX = dY @ W.double()

    def part(lo, hi):
        o = {"dW": dY[lo:hi].t() @ X[lo:hi], "db": dY[lo:hi].sum(0)}
        if masked:
            o["r0"], o["r1"] = dX[lo:hi].sum(0), (dX[lo:hi] * xhat[lo:hi]).sum(0)
        return o
    ref = dict(part(0, P), dX=dX, part=part)
    return dict(Y=Y, Yp=Yp, affp=affp, W=W, ldw=ldw, w_store=w_store, coef=coef, dz_args=dz_args, keep=keep, ldc=ldc, ldp=ldp), ref
