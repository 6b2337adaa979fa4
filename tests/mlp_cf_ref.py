"""Fixed operands and fp64 statements of the closed-form / output-free conv1x1 entry points: pn2_conv1x1_bwd_cf
(split_bwd_cf_kernel with cf_prep_kernel / cf_finish_kernel, csrc/mlp_res.hip), pn2_conv1x1_bwd_first (split_bwd_res_kernel,
FUSE0) and pn2_conv1x1_wgrad_cf (wgrad_first_cf_kernel, csrc/mlp.hip) with and without dZ.  Written from the formulas of
include/pn2.h in the style of tests/mlp_ref.py (whose guards, frames and BatchNorm blocks are used as they are): for clarity,
not speed; every function takes tensors of any device and answers on that device.

NO DECISION IN THE PATH, as in mlp_ref: the ReLU mask is that of the given previous output on both sides and the pooled rows
are those of the given arg.

BUFFER RULES.  Every input holds NaN from round4(C) to its pitch (nobody may read there); outputs come from mlp_ref.guarded
(dX) or mlp_ref.framed (dW, dW0: accumulated into random initial contents).

COEFFICIENT BLOCKS.  "random": mlp_ref.draw_coef (q1, q0 ~ 1e-3: the BatchNorm terms are a small correction).  "bigq1": q1 of
the order of c0, so that the closed-form terms carry the result.  "self": the block a real BatchNorm backward has --
coef_block(r0, r1, P, gamma, mean, invstd) on THIS layer's fp64 reductions with mean / invstd the true column statistics of
Y = X W^T + b, so that sum dY = 0 and sum dY yhat = 0 hold and the c0, q1 and q0 terms cancel in every column sum.  The
statement is always evaluated on the float32-rounded block the kernel is handed.

BOUNDS (``bound``).  3e-6 of the reference tensor's largest entry -- what tests/test_mlp_gpu.py and test_mlp_seams_gpu.py hold
this operand generator to.  Where that largest entry is itself a cancelled sum ("self", "bigq1") the project's rule for such
sums applies: max(3e-6, 4 e32) with e32 the error of a plain float32 torch evaluation of the textbook form on the same
operands (``textbook_f32``: dY per row in fp32, then dY^T X and dY W) -- stock arithmetic, not this library.
"""
import torch

import mlp_ref as R

EPS = 1e-5
NAN = float("nan")
TOL = 3e-6


def nan_rows(rows, C, ld, values):
    """[rows, ld]: `values` in the leading C columns, zeros up to round4(C), NaN behind."""
    t = torch.full((rows, ld), NAN, device=values.device, dtype=values.dtype)
    t[:, :C] = values
    t[:, C:R.round4(C)] = 0
    return t


def poison_pitch(t, C):
    t[:, R.round4(C):] = NAN
    return t


def scatter_rows(dzp, arg, Kp):
    """fp64 D [G Kp, C]: D[g Kp + arg[g, c], c] = dzp[g, c], zero elsewhere (the gradient behind a max over Kp rows)."""
    G, C = dzp.shape
    D = torch.zeros(G, Kp, C, device=dzp.device, dtype=torch.float64)
    D.scatter_(1, arg.long().unsqueeze(1), dzp.double().unsqueeze(1))
    return D.view(G * Kp, C)


def true_stats(Y):
    """Column mean and 1 / sqrt(biased variance + eps) of an fp64 Y."""
    mean = Y.mean(0)
    return mean, 1.0 / torch.sqrt(((Y - mean) ** 2).mean(0) + EPS)


def self_block(D, Y, gamma):
    """fp64 [4, C]: the coefficient block of a training-mode BatchNorm backward on this very layer (module docstring)."""
    mean, invstd = true_stats(Y)
    r0, r1 = D.sum(0), (D * (Y - mean) * invstd).sum(0)
    return R.coef_block(r0, r1, Y.shape[0], gamma, mean, invstd)


# ------------------------------------------------------------------------------------------------ statements

def layer_statement(D, coef, W, bias, X, mask=None, xhat=None):
    """fp64: Y = X W^T + b, dY = c0 D + q1 (Y - mean) + q0, dX = (dY W) o mask, dW = dY^T X and, with xhat, the two
    reductions of the masked dX.  coef: [4, C_out] rows c0, q1, q0, mean."""
    Y = X @ W.double().t() + bias.double()
    dY = R.dy_of(coef.double(), D, Y)
    dX = dY @ W.double()
    if mask is not None:
        dX = dX * mask
    out = {"Y": Y, "dY": dY, "dX": dX, "dW": dY.t() @ X}
    if xhat is not None:
        out["r0"], out["r1"] = dX.sum(0), (dX * xhat).sum(0)
    return out


def first_dw_statement(part, coef0, W0, b0, x0):
    """fp64 dW0 [M, N] of a first layer from part = dZ^T x0 and the input's moments (include/pn2.h, pn2_conv1x1_wgrad_cf):
    c0 part + q1 (W0 S + (b0 - mean) s^T) + q0 s^T with S = x0^T x0, s = sum_p x0_p."""
    c0, q1, q0, mu = coef0.double()
    S, s = x0.t() @ x0, x0.sum(0)
    return c0[:, None] * part + q1[:, None] * (W0.double() @ S + (b0.double() - mu)[:, None] * s[None, :]) + q0[:, None] * s[None, :]


def textbook_f32(D, coef, W, bias, X, mask=None, xhat=None):
    """The textbook form in plain float32 torch arithmetic: dY per row in fp32, then dY^T X and dY W (module docstring)."""
    c0, q1, q0, mu = coef.float()
    Xf, Wf = X.float(), W.float()
    Y = Xf @ Wf.t() + bias.float()
    dY = c0 * D.float() + q1 * (Y - mu) + q0
    dX = dY @ Wf
    if mask is not None:
        dX = dX * mask
    out = {"dX": dX, "dW": dY.t() @ Xf}
    if xhat is not None:
        out["r0"], out["r1"] = dX.sum(0), (dX * xhat.float()).sum(0)
    return out


def bound(kind, e32):
    """The bound of a tensor in a case of coefficient kind `kind` (module docstring); e32: the error of textbook_f32's
    tensor, measured exactly as the error under test is."""
    return TOL if kind == "random" else max(TOL, 4.0 * e32)


# ------------------------------------------------------------------------------------------------ pn2_conv1x1_bwd_cf

ARG_MODES = ("random", "row0", "last", "same", "planted")


def draw_arg(g, G, C, Kp, mode, dev):
    if mode == "row0":
        return torch.zeros(G, C, device=dev, dtype=torch.int32)
    if mode == "last":
        return torch.full((G, C), Kp - 1, device=dev, dtype=torch.int32)
    if mode == "same":                                              # every channel of a group at the same row
        return torch.randint(0, Kp, (G, 1), device=dev, dtype=torch.int32, generator=g).expand(G, C).contiguous()
    a = torch.randint(0, Kp, (G, C), device=dev, dtype=torch.int32, generator=g)
    if mode == "planted":                                           # both sides of the 32-row chunk boundary inside a group
        assert Kp >= 64
        a[:, 0::3], a[:, 1::3] = 31, 32
    return a


def bwd_cf_case(dev, P, co, ci, Kp, seed, coef="random", arg_mode="random", ldo=None, ldp=None, ldw=None, tail_from=None,
                zero_dzp=False, dead=None):
    """Fixed operands of ONE pn2_conv1x1_bwd_cf call and its fp64 statement.  Inputs: dZp / arg [P / Kp, ldo] (arg's pad holds
    large row numbers), prev_Y [P, ldp] with its affine block (both signs of the scale), W [co, ci] at pitch ldw, bias, the
    coefficient block (a kind of the module docstring, or a float32 tensor [4 co] to use as it is).  X = float32(max(fma(prev_Y -
    mean, scale, beta), 0)).  tail_from: rows >= it of prev_Y and their groups of dZp are scaled by mlp_ref.TAIL_SCALE.
    zero_dzp: dZp = 0 and q1 = q0 = 0 (everything must come out exactly zero).  dead: an input channel with scale 0 and
    beta <= 0, a column of X that is exactly zero."""
    g, rnd = R._rnd(dev, seed)
    G = P // Kp
    assert G * Kp == P
    ldo, ldp, ldw = ldo or co, ldp or ci, ldw or ci
    ypv = rnd(P, ci) * 1.5 + 0.3
    dzv = rnd(G, co)
    dzv[rnd(G, co) > 0.5] = 0.0                                     # (outputs that were <= 0 carry nothing)
    if zero_dzp:
        dzv.zero_()
    if tail_from is not None:
        assert tail_from % Kp == 0
        ypv[tail_from:] *= R.TAIL_SCALE
        dzv[tail_from // Kp:] *= R.TAIL_SCALE
    Yp, dzp = nan_rows(P, ci, ldp, ypv), nan_rows(G, co, ldo, dzv)
    arg = torch.full((G, ldo), 0x7FFFFF00, device=dev, dtype=torch.int32)
    arg[:, :co] = draw_arg(g, G, co, Kp, arg_mode, dev)
    affp = R.draw_affine(rnd, ci, ci, dev)
    affp[ci:2 * ci][::7] *= -1.0
    if dead is not None:
        affp[ci + dead] = 0.0
        affp[2 * ci + dead] = -affp[2 * ci + dead].abs()
    w_store = nan_rows(co, ci, ldw, rnd(co, ci) * 0.2)
    W, bias = w_store[:, :ci], rnd(co) * 0.1
    gamma = rnd(co) * 0.5 + 1.0
    gamma[::5] *= -1.0
    ap = affp.view(4, ci)
    X, z = R.bn_relu(Yp[:, :ci], ap)
    mask, xhat = z > 0, (Yp[:, :ci] - ap[0]).double() * ap[3].double()
    D = scatter_rows(dzp[:, :co], arg[:, :co], Kp)
    kind = coef if isinstance(coef, str) else "random"
    if not isinstance(coef, str):
        block = coef
    elif coef == "self":
        block = self_block(D, X @ W.double().t() + bias.double(), gamma).float().reshape(-1)
    else:
        block = R.draw_coef(rnd, co, co, dev)
        if coef == "bigq1":
            block[co:2 * co] = rnd(co) * 0.5
        if zero_dzp:
            block[co:3 * co] = 0.0
    cf = block.view(4, co)
    ref = layer_statement(D, cf, W, bias, X, mask, xhat)
    ref.update(X=X, D=D, mask=mask, xhat=xhat, f32=textbook_f32(D, cf, W, bias, X, mask, xhat), kind=kind)
    return dict(dzp=dzp, arg=arg, ldo=ldo, Kp=Kp, Yp=Yp, ldp=ldp, affp=affp, W=W, w_store=w_store, ldw=ldw, bias=bias, coef=block,
                gamma=gamma), ref


# ------------------------------------------------------------------------------------------------ pn2_conv1x1_bwd_first + wgrad_cf

def draw_x0(rnd, P, N, ld, zero_to, dev):
    """Input rows [P, ld] of a first layer: N columns with non-zero means (as test_first_layer_weight_gradient_closed_form
    draws them), zeros up to column zero_to and NaN behind."""
    v = rnd(P, N) * torch.linspace(0.3, 2.0, N, device=dev) + torch.linspace(-1.0, 3.0, N, device=dev)
    t = torch.full((P, ld), NAN, device=dev)
    t[:, :zero_to] = 0
    t[:, :N] = v
    return t


def nan_weight(rnd, M, N, dev):
    """W [M, N] * 0.3 as columns of an [M, N + 3] matrix with NaN in the three others (ldw >= N is all the contract asks)."""
    store = torch.full((M, N + 3), NAN, device=dev)
    store[:, :N] = rnd(M, N) * 0.3
    return store


def first_case(dev, P, co, ci, N0, ld0, seed, tail_from=None, wide=False, coef=None):
    """Fixed operands of pn2_conv1x1_bwd_first (a dense masked layer co x ci, mlp_ref.fixed_layer_case, behind a first layer
    N0 -> ci on the rows X0 [P, ld0]) followed by pn2_conv1x1_wgrad_cf without dZ, and the fp64 statement: this layer's dW and
    reductions, and the first layer's dW0 = c0 dZ1^T x0 + q1 (W0 S + (b0 - mean0) s^T) + q0 s^T with dZ1 the masked dX.
    wide: dZ / Y and prev_Y at pitches + 4 / + 8 with NaN behind the width."""
    c, ref = R.fixed_layer_case(dev, P, co, ci, 0, seed, tail_from=tail_from, coef=coef, ldc=co + 4 if wide else None,
                                ldp=ci + 8 if wide else None)
    for t, C in ((c["Y"], co), (c["keep"][0], co), (c["Yp"], ci)):
        poison_pitch(t, C)
    g, rnd = R._rnd(dev, seed + 77)
    X0 = draw_x0(rnd, P, N0, ld0, 12, dev)                        # (the contract: 12 columns are read, the pad columns are zero)
    w0_store = nan_weight(rnd, ci, N0, dev)
    b0, coef0 = rnd(ci) * 0.1, R.draw_coef(rnd, ci, ci, dev)
    x0 = X0[:, :N0].double()
    ref = dict(ref, dW0=first_dw_statement(ref["dX"].t() @ x0, coef0.view(4, ci), w0_store[:, :N0], b0, x0))
    return dict(c, X0=X0, ld0=ld0, N0=N0, W0=w0_store[:, :N0], w0_store=w0_store, ldw0=N0 + 3, b0=b0, coef0=coef0), ref


SELF_MIN_ROWS, SELF_MIN_COLUMNS = 127, 3


def wgrad_cf_kinds(P, N):
    """The coefficient blocks a pn2_conv1x1_wgrad_cf case of P rows and N input columns is run with: the random one always,
    the self-consistent one where it leaves a gradient with a scale -- from 127 rows on (the true statistics of a handful of
    rows make dY vanish; P = 1: identically) and from 3 input columns on (N = 1: Y is an affine function of the one column
    and dW = c0 r1 eps invstd / w, the residue of the eps under the root: tests/test_mlp_cf_ref_cpu.py)."""
    return ("random", "self") if P >= SELF_MIN_ROWS and N >= SELF_MIN_COLUMNS else ("random",)


def wgrad_cf_case(dev, P, M, N, ldx, ldz, seed, coef="random"):
    """Fixed operands of pn2_conv1x1_wgrad_cf WITH dZ -- X [P, ldx] (columns with non-zero means), dZ [P, ldz], W [M, N] at
    pitch N + 3, bias, the coefficient block -- and the fp64 statement dW = dY^T X, dY = c0 dZ + q1 (X W^T + b - mean) + q0."""
    g, rnd = R._rnd(dev, seed)
    X = draw_x0(rnd, P, N, ldx, N, dev)                           # (ldx >= N is all the contract asks: NaN from column N on)
    dZ = nan_rows(P, M, ldz, rnd(P, M))
    w_store = nan_weight(rnd, M, N, dev)
    W, bias = w_store[:, :N], rnd(M) * 0.1
    gamma = rnd(M) * 0.5 + 1.0
    gamma[::5] *= -1.0
    x, D = X[:, :N].double(), dZ[:, :M].double()
    if coef == "self":
        block = self_block(D, x @ W.double().t() + bias.double(), gamma).float().reshape(-1)
    else:
        block = R.draw_coef(rnd, M, M, dev)
    ref = layer_statement(D, block.view(4, M), W, bias, x)
    ref.update(f32=textbook_f32(D, block.view(4, M), W, bias, x), kind=coef,
               closed=first_dw_statement(D.t() @ x, block.view(4, M), W, bias, x))
    return dict(X=X, ldx=ldx, dZ=dZ, ldz=ldz, W=W, w_store=w_store, ldw=N + 3, bias=bias, coef=block), ref


# ------------------------------------------------------------------------------------------------ case tables

def bwd_cf_table(Rm, g, co, ci):
    """{name: (P, Kpool, bwd_cf_case keywords, output pitches)} of the pn2_conv1x1_bwd_cf cases, from Rm = the row count
    from which the call is taken (PN2_RES_MIN_ROWS) and g = the grid cap of launch_split_bwd_cf.  The names do not depend
    on the two values."""
    up = lambda n, m: -(-n // m) * m
    k = max((Rm // 32 - (g - 1)) // g + 1, 1)                       # 32 (k g + g - 1): the first such row count above Rm
    pow2 = 1 << (max(Rm, 1024) - 1).bit_length()
    t = {"rows-R": (Rm, 32, {}, {}),
         "rows-R+32": (Rm + 32, 32, dict(tail_from=Rm), {}),          # one workgroup takes an extra trip: its chunk weighs 32 x
         "rows-all-but-one-extra-trip": (32 * (k * g + g - 1), 32, {}, {})}
    for Kp in (32, 64, 128, 256, 1024):
        t["kpool-%d" % Kp] = (up(Rm, Kp), Kp, {}, {})
    t["kpool-one-group"] = (pow2, pow2, {}, {})
    for mode in ARG_MODES:
        t["arg-" + mode] = (up(Rm, 64), 64, dict(arg_mode=mode), {})
    t["exact-zero"] = (Rm, 32, dict(zero_dzp=True), {})
    t["exact-dead-column"] = (Rm, 32, dict(dead=5), {})
    t["pitch-narrow"] = (Rm, 32, dict(ldo=co + 8, ldp=ci + 4, ldw=ci + 3), dict(ldxo=ci + 4, lddw=ci + 3))
    t["pitch-wide"] = (up(Rm, 64), 64, dict(ldo=co + 8, ldp=ci + 32, arg_mode="planted"), dict(ldxo=ci + 32))
    t["coef-self"] = (Rm, 32, dict(coef="self"), {})
    t["coef-self-k64"] = (up(Rm, 64), 64, dict(coef="self", arg_mode="planted"), {})
    t["coef-bigq1"] = (Rm, 32, dict(coef="bigq1"), {})
    return t


BWD_CF_NAMES = tuple(bwd_cf_table(32768, 256, 128, 96))
SMALL_N = ("1", "2", "3", "4", "5", "28", "29", "32", "33", "g-1", "g", "g+1", "2g+1")


def small_n(name, g):
    """The chunk / tile count a name of SMALL_N stands for."""
    return {"g-1": g - 1, "g": g, "g+1": g + 1, "2g+1": 2 * g + 1}.get(name) or int(name)
