"""Operands, fp64 statements, a-priori bounds and float32 emulations of the small kernels between the GEMMs: pn2_bn_relu_max,
pn2_bn_pool_select, pn2_pool_bwd_reduce / _ld / _rec, pn2_relu_bwd_reduce, pn2_bn_finalize / pn2_bn_bwd_coef, and their
PointNet v1 / DenseCls relatives (pn2_bn_max, pn2_pool_bwd_reduce_noact, pn2_group_colsum, pn2_bn_bwd_reduce_noact_dense).
A test helper in the style of tests/mlp_ref.py, written from the formulas of include/pn2.h, for clarity, not speed.  Every
operand set is drawn on the CPU with numpy from a seed, so tests/test_bn_pool_ref_cpu.py (no GPU) and
tests/test_bn_pool_gpu.py see the SAME numbers; the statements are numpy fp64.

LATTICE OPERANDS (``lattice_case``, the forward kernels).  Y and mean are multiples of 1/64 in [-8, 8], scale a multiple of
1/8 in [-2, 2] (|scale| >= 1/4 or exactly 0), beta a multiple of 1/16 in [-1, 1].  y - mean is a multiple of 1/64 below 16,
its product with scale a multiple of 1/512 below 32, and so is the sum with beta: fewer than 2^15 units of 1/512, so
fma(y - mean, scale, beta) is EXACT in float32 and equals the fp64 value -- no rounding exists that could blur a tie.
out = max_k max(z_k, 0) and arg = the first k attaining it (numpy's argmax: row 0 of an all-equal group, as torch.max) are
compared bit for bit.  Planted per case, where K allows (``plants`` says where): the maximum repeated at k0 + RPW and at
k0 + 1, the maximum repeated in another quarter of K (the ksplit form), a group whose rows are all equal, a group whose
values are all <= 0 (out = 0, arg = 0), channels with negative scale (the smallest y wins) and with zero scale.  (In
bn_relu_max_kernel a row-lane visits k_lo + rsub, + RPW, ...: k0 + RPW is the SAME row-lane's next visit -- its strict `>` --
and k0 + 1 the neighbouring row-lane -- the shuffles' "equal and smaller k"; both are planted.)  Free entries stay inside
[-500/64, 500/64], the planted extremes are +-8: no free entry can beat a plant.

RANDOM OPERANDS (``reduce_case``, the reductions).  dOut is a non-zero multiple of 1/256 in [-4, 4] (so sum dZ is exact in
fp64 in any order: red0 is compared BIT for BIT besides its bound).  Y holds a value at the rows `arg` names only, every
other element is 1e30: a gather of the wrong row cannot hide.  The BatchNorm weight per channel cycles through eight kinds
(``KINDS``): gamma = 1, beta = 0 (a fresh BatchNorm); a negative gamma; exactly 0; exactly the branch threshold
(1 + |beta|) / 4; the float32 just below it; minus the float32 just above it; +-0.01 (far below); a positive random one.
beta is a multiple of 1/16, so the threshold is a float32 number, and the three threshold kinds have invstd in {1/2, 1, 2}:
scale = gamma * invstd and scale / invstd are then exact and the branch the kernel takes is known, not a matter of
rounding.  Every third entry (g C + c = 0 mod 3) of a channel with gamma != 0 has y* chosen so that z <= 0: out = 0 with
dOut != 0, the mask matters on at least a fifth of the entries; the others have z > 0.  arg of every other channel of the
LAST group is K - 1: the last row of Y.  `out` is the fp64 statement max(fma(fl32(y* - mean), scale, beta), 0) rounded to
float32.

STATEMENTS (fp64; mean, scale, invstd are the block's float32 values, as the kernels read them):
  dZp = dOut * (out > 0);  red0 = sum dZp;  red1 = sum dZp * xhat,  xhat = (y* - mean) * invstd  (y* - mean EXACT).
The dense form (pn2_relu_bwd_reduce) is the same with K = 1 and every row of Y real.  The _rec form reads y* from the
{value, row} record; a channel with scale == 0 takes y = bias + W . relu(bn(prev_Y[g K])) instead (``rec_y``).

BOUNDS -- counted, none fitted to a result.  u = 2^-24; n = terms of the sum.
  red0:  (n + 8) 2^-53 sum |dZ|: fp64 additions of float32 terms (n - 1 in the thread / workgroup / replica tree, a few more
         when the replicas are folded).  0 on these dyadic dOut: also compared exactly.
  red1, gather branch:  term = fl(dz * fl(fl(y - mean) * invstd)): three float32 roundings, (1 + u)^3 - 1 <= 3.01 u, so
         3.01 u sum |dZ xhat|, plus the fp64 accumulation term (n + 8) 2^-53 sum |dZ xhat| and the red0 term.
  red1, `out` branch:  the kernel forms ga = fl(scale / invstd), rga = fl(1 / ga), term = fl(dz * fl(fl(out - beta) * rga)).
         With gamma = scale / invstd EXACT (what the block holds), z = fl(y - mean) * scale + beta:
           out = z (1 + e1);  fl(y - mean) = (y - mean)(1 + e0)  =>  (out - beta) / gamma = xhat (1 + e0) + e1 z / gamma
         and then out - beta (e2), scale / invstd (e3), its reciprocal (e4), the two products (e5, e6) each put one rounding
         on the whole: |term - dz xhat| <= u |dz| (6 |xhat| + |e1 / u| |z| / |gamma|) to first order -- A = 6 (e0, e2 .. e6).
         The kernel takes `out` as an INPUT, so only |out - z| counts: B = 1.  This file's `out` is the fp64 value rounded to
         float32 -- a double rounding that can name the other float32 neighbour than fmaf would (the header's precondition is
         bit equality with the kernel's own fmaf; here the kernel never sees those bits) -- and is within (u + 2^-53) |z| of z
         either way: the bound covers it through the allowance below, not through B.  Second order: (1 + u)^7 - 1 - 7 u <
         22 u^2, and |z| <= |out| (1 + 2 u): both far inside the 1 % allowance the gather form's 3.01 carries too.  With
         |out| <= |out| + |beta| (the form the bound is stated in):
           1.01 u sum |dZ| (A |xhat| + B (|out| + |beta|) / |gamma|),  A = 6, B = 1,  plus the fp64 accumulation term.
  recomputed y (_rec, zero scale): a C_in-term float32 fma chain on bias, 1.05 (C_in + 4) u (|bias| + sum |w x|) as
         tests/scatter_ref.py derives it (the x entering it carry one rounding of their own, inside its k <= 3); it enters
         xhat times invstd, then the three roundings of the gather form: 3.01 u sum |dZ xhat| + 1.01 invstd sum |dZ| e_y.
  affine / coefficient / running entries: the kernels evaluate the fp64 formulas of mlp_ref.affine_block / coef_block with
         reciprocals where the statement divides (a few 2^-53 apart) and round ONCE to float32: the result is the rounded
         statement or, where those 2^-53 cross a rounding boundary, its neighbour -- within one float32 ulp (``ulps``).
  pn2_group_colsum: an fp32 sum of n terms fma(c0, dz, fma(q1, y - mean, q0)) of three roundings each:
         scatter_ref.bound(n, sum |terms|) with |term| <= |c0 dz| + |q1 (y - mean)| + |q0|.

EMULATIONS (``emulate_reduce``, ``emulate_relu_max``, ``emulate_pool_select``): the kernels' arithmetic in numpy float32, both
xhat formulas and the branch rule as include/pn2.h states them, with the seven MUTANTS of tests/test_bn_pool_ref_cpu.py: the
evidence that the assertions of the GPU test would catch a subtly wrong kernel.
"""
import numpy as np

from mlp_ref import SENTINEL, STAT_REPLICAS, affine_block, check_guards, coef_block, guarded, replicate, round4  # noqa: F401 (re-exported)
import scatter_ref

U32 = 2.0 ** -24
U64 = 2.0 ** -53
POISON = np.float32(1e30)
A_OUT, B_OUT = 6, 1                  # the two integers of the `out` branch bound (module docstring)
f32, f64 = np.float32, np.float64


def lane_geometry(C):
    """(LPR, RPW, gx) of bn_relu_max_kernel: LPR = 2^ceil(log2(round4(C) / 4)) lanes per row capped at 64, RPW = 64 / LPR
    row-lanes per wave, gx column blocks."""
    cg = round4(C) // 4
    lpr = 1
    while lpr < cg and lpr < 64:
        lpr *= 2
    return lpr, 64 // lpr, -(-cg // lpr)


def block(mean, scale, beta, invstd):
    """float32 [4 * round4(C)] affine block [mean | scale | beta | invstd], pad entries zero."""
    C = len(mean)
    b = np.zeros((4, round4(C)), f32)
    b[0, :C], b[1, :C], b[2, :C], b[3, :C] = mean, scale, beta, invstd
    return b.reshape(-1)


def rows(P, C, ld, values, poison=POISON, pad=0.0):
    """float32 [P, ld]: `values` in the leading C columns, `pad` up to round4(C), `poison` behind (mlp_ref._rows)."""
    t = np.full((P, ld), poison, f32)
    t[:, :C] = values
    t[:, C:round4(C)] = pad
    return t


def fma32(a, b, c):
    """fmaf on float32 arrays: the fp64 product is exact; its sum with c is rounded to fp64, then to float32 (exact on the
    lattice; elsewhere a double rounding that can differ from fmaf by one ulp -- module docstring)."""
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def ulps(got, ref64):
    """Distance of float32 `got` from the fp64 statement rounded to float32, in float32 ulps of that value."""
    r = np.asarray(ref64, f64).astype(f32)
    sp = np.maximum(np.spacing(np.abs(r)), np.spacing(f32(1.1754944e-38)))
    return np.abs(got.astype(f64) - r.astype(f64)) / sp.astype(f64)


# ================================================================================================ lattice operands (forward)

def lattice_case(seed, G, K, C, relu=True, rpw=None, tie_step=None):
    """Lattice operands of one pn2_bn_relu_max / pn2_bn_max call (module docstring) and its exact statement.  rpw: the
    row-lane count the first planted tie steps over (default: lane_geometry(C)); tie_step overrides it (pn2_bn_max: any
    two rows below 64 sit on different lanes).  Returns a dict: Y [G, K, C] float32, aff (block), out [G, C] float32,
    arg [G, C] int32, plants {name: (group, k0, k1) or group}."""
    rng = np.random.default_rng(seed)
    mean = (rng.integers(-128, 129, C) / 64.0).astype(f32)
    mag = rng.integers(2, 17, C) / 8.0
    c_idx = np.arange(C) + seed
    scale = np.where(c_idx % 5 == 3, 0.0, np.where(c_idx % 5 == 1, -mag, mag)).astype(f32)
    beta = (rng.integers(-16, 17, C) / 16.0).astype(f32)
    Y = (rng.integers(-500, 501, (G, K, C)) / 64.0).astype(f32)
    rpw = lane_geometry(C)[1] if rpw is None else rpw
    step = tie_step or rpw
    kq = (K + 3) >> 2
    ext = np.where(scale < 0, -8.0, 8.0).astype(f32)              # the winning pre-BN value per channel (z >= 6 / 4 - 1 > 0)
    plants = {}
    # later plants are applied first: with fewer than four groups the ties (applied last) survive
    if K > 1:
        g = 3 % G                                                   # every z <= 0: (y - mean) = -sign(scale) (4 + r), |scale| >= 1/4, |beta| <= 1
        r = rng.integers(0, 129, (K, C)) / 64.0
        Y[g] = (mean + np.where(scale < 0, 1.0, -1.0) * (4.0 + r)).astype(f32)
        plants["all_nonpositive"] = g
        g = 2 % G
        Y[g] = Y[g, 0]
        plants["all_equal"] = g
        if K >= 32 and kq < K:
            g, k0 = 1 % G, min(2, kq - 1)
            k1 = k0 + kq * (2 if k0 + 2 * kq < K else 1)
            Y[g, k0], Y[g, k1] = ext, ext
            plants["tie_quarter"] = (g, k0, k1)
        if step < K:
            k0 = 1 if step + 1 < K else 0
            Y[0, k0], Y[0, k0 + step] = ext, ext                  # k0 + RPW: the same row-lane's next visit (its strict >)
            if k0 + 1 < K:
                Y[0, k0 + 1] = ext                                  # and the neighbouring row-lane (the shuffles' "equal and smaller k")
            plants["tie_lane"] = (0, k0, k0 + step)
    z = (Y - mean).astype(f64) * scale.astype(f64) + beta.astype(f64)
    assert np.array_equal(z.astype(f32).astype(f64), z)           # the lattice: exact in float32
    out, arg = pool_fwd(Y, mean, scale, beta, relu)
    out = out.astype(f32)
    return dict(G=G, K=K, C=C, Y=Y, mean=mean, scale=scale, beta=beta, aff=block(mean, scale, beta, np.ones(C, f32)), out=out, arg=arg,
                plants=plants, relu=relu)


def pool_fwd(Y, mean, scale, beta, relu=True):
    """fp64 statement of the pooled forward: Y [G, K, C] -> out [G, C] = max_k act(z_k), z = (y - mean) scale + beta, and arg =
    the first k attaining it (numpy's argmax names the FIRST index of the maximum)."""
    z = (Y.astype(f64) - mean.astype(f64)) * scale.astype(f64) + beta.astype(f64)
    o = np.maximum(z, 0.0) if relu else z
    return o.max(1), o.argmax(1).astype(np.int32)


def emulate_relu_max(c, mutant=None):
    """bn_relu_max_kernel / bn_max_kernel in float32: z = fmaf(y - mean, scale, beta), the ReLU, the maximum and the first row
    attaining it.  mutant 6: the LAST row attaining it."""
    z = fma32((c["Y"] - c["mean"]).astype(f32), c["scale"], c["beta"])
    o = np.maximum(z, f32(0)) if c["relu"] else z
    out = o.max(1)
    if mutant == 6:
        arg = c["K"] - 1 - o[:, ::-1].argmax(1)
    else:
        arg = o.argmax(1)
    return out, arg.astype(np.int32)


def record_case(seed, G, K, C):
    """Drawn {value, row} records of pn2_bn_pool_select on the lattice, with its statement: out = relu(fma(v - mean, scale,
    beta)), arg = the recorded row, 0 where scale == 0 (whatever the record holds: its rows are drawn in [1, K))."""
    rng = np.random.default_rng(seed)
    mean = (rng.integers(-128, 129, C) / 64.0).astype(f32)
    mag = rng.integers(2, 17, C) / 8.0
    c_idx = np.arange(C) + seed
    scale = np.where(c_idx % 5 == 3, 0.0, np.where(c_idx % 5 == 1, -mag, mag)).astype(f32)
    beta = (rng.integers(-16, 17, C) / 16.0).astype(f32)
    v = (rng.integers(-512, 513, (G, C)) / 64.0).astype(f32)
    row = rng.integers(1 if K > 1 else 0, K, (G, C)).astype(np.int32)
    row[::2, ::7] = 0
    rec = np.empty((G, C, 2), f32)
    rec[..., 0] = v
    rec[..., 1] = row.view(f32)
    z = (v - mean).astype(f64) * scale.astype(f64) + beta.astype(f64)
    assert np.array_equal(z.astype(f32).astype(f64), z)
    return dict(G=G, K=K, C=C, rec=rec, v=v, row=row, mean=mean, scale=scale, beta=beta, aff=block(mean, scale, beta, np.ones(C, f32)),
                out=np.maximum(z, 0.0).astype(f32), arg=np.where(scale == 0, 0, row).astype(np.int32))


def emulate_pool_select(c, mutant=None):
    """bn_pool_select_kernel in float32.  mutant 7: row 0 not forced for a zero scale."""
    out = np.maximum(fma32((c["v"] - c["mean"]).astype(f32), c["scale"], c["beta"]), f32(0))
    arg = c["row"] if mutant == 7 else np.where(c["scale"] == 0, 0, c["row"])
    return out, arg.astype(np.int32)


# ================================================================================================ random operands (reductions)

KINDS = ("fresh", "negative", "zero", "at", "below", "above_neg", "small", "positive")


def reduce_case(seed, G, K, C, dense=False, C_in=None):
    """Random operands of one pn2_pool_bwd_reduce / _ld / _rec call (dense: of pn2_relu_bwd_reduce, K = 1 and every row of Y
    real) -- module docstring.  Arrays are dense [.., C]; the tests lay them out at their pitches.  C_in: also the _rec
    form's W, bias, prev_Y rows g K, prev_aff and the recomputed y of the zero-scale channels."""
    assert not dense or K == 1
    rng = np.random.default_rng(seed)
    kind = (np.arange(C) + seed) % 8
    beta = (rng.integers(-16, 17, C) / 16.0).astype(f32)
    beta[kind == 0] = 0.0
    zero_pos = (np.arange(C) // 8 + seed) % 2 == 0
    beta[kind == 2] = np.where(zero_pos, 0.5, -0.25)[kind == 2]    # zero scale: out = relu(beta) on every row
    thr = ((1.0 + np.abs(beta.astype(f64))) / 4.0).astype(f32)     # a float32 number: beta is a multiple of 1/16
    assert np.array_equal(thr.astype(f64), (1.0 + np.abs(beta.astype(f64))) / 4.0)
    gamma = rng.uniform(0.5, 2.0, C).astype(f32)
    gamma[kind == 0] = 1.0
    gamma[kind == 1] *= -1.0
    gamma[kind == 2] = 0.0
    gamma[kind == 3] = thr[kind == 3]
    gamma[kind == 4] = np.nextafter(thr, f32(0))[kind == 4]
    gamma[kind == 5] = -np.nextafter(thr, f32(np.inf))[kind == 5]
    gamma[kind == 6] = np.where(np.arange(C) % 16 < 8, 0.01, -0.01).astype(f32)[kind == 6]
    invstd = rng.uniform(0.5, 2.0, C).astype(f32)
    dy = (kind >= 3) & (kind <= 5)
    invstd[dy] = rng.choice(np.array([0.5, 1.0, 2.0], f32), C)[dy]
    mean = (rng.standard_normal(C) * 0.5).astype(f32)
    scale = (gamma.astype(f64) * invstd.astype(f64)).astype(f32)  # as bn_finalize_channel forms it
    # y*: z > 0 on the live entries, z <= 0 on every third
    idx = np.arange(G)[:, None] * C + np.arange(C)[None, :]
    masked = (idx % 3 == 0)
    nz = gamma != 0
    g64 = np.where(nz, gamma, 1).astype(f64)
    r = rng.uniform(0.1, 2.0, (G, C))
    away = np.abs(beta.astype(f64)) / np.abs(g64)
    xh = np.where(masked, -np.sign(g64) * (away + 0.5 + r), np.sign(g64) * (away + r))
    xh = np.where(nz[None, :], xh, rng.standard_normal((G, C)))
    ystar = (mean.astype(f64) + xh / invstd.astype(f64)).astype(f32)
    arg = rng.integers(0, K, (G, C)).astype(np.int32)
    arg[G - 1, ::2] = K - 1                                         # the last row of the last group
    arg[:, ~nz] = 0                                                 # zero scale names row 0 (pn2.h)
    Y = np.full((G * K, C), POISON, f32)
    cols = np.broadcast_to(np.arange(C)[None, :], (G, C))
    Y[np.arange(G)[:, None] * K + arg, cols] = ystar
    z = (ystar - mean).astype(f32).astype(f64) * scale.astype(f64) + beta.astype(f64)
    out = np.maximum(z, 0.0).astype(f32)
    live = out > 0
    assert np.array_equal(live[:, nz], ~masked[:, nz]) and np.array_equal(live[:, ~nz], np.broadcast_to(beta > 0, (G, C))[:, ~nz])
    dOut = rng.integers(-1024, 1025, (G, C))
    dOut = (np.where(dOut == 0, 1, dOut) / 256.0).astype(f32)
    c = dict(G=G, K=K, C=C, kind=kind, gamma=gamma, beta=beta, mean=mean, invstd=invstd, scale=scale, aff=block(mean, scale, beta, invstd),
             Y=Y, ystar=ystar, arg=arg, out=out, dOut=dOut, dense=dense)
    if C_in:
        pm = (rng.standard_normal(C_in) * 0.2).astype(f32)
        ps = (np.abs(rng.standard_normal(C_in)) * 0.5 + 0.3).astype(f32)
        pb = (rng.standard_normal(C_in) * 0.3).astype(f32)
        c["prev_aff"] = block(pm, ps, pb, np.ones(C_in, f32))
        c["W"] = (rng.standard_normal((C, C_in)) * 0.2).astype(f32)
        c["bias"] = (rng.standard_normal(C) * 0.1).astype(f32)
        c["prev0"] = (rng.standard_normal((G, C_in)) * 1.5 + 0.3).astype(f32)      # prev_Y[g K, :]
        x = np.maximum(fma32((c["prev0"] - pm).astype(f32), ps, pb), f32(0))         # the activation the kernel stages
        t = x.astype(f64)[:, None, :] * c["W"].astype(f64)[None, :, :]              # [G, C, C_in]
        c.update(C_in=C_in, x=x, rec_y=c["bias"].astype(f64) + t.sum(2), rec_abs=np.abs(c["bias"].astype(f64)) + np.abs(t).sum(2))
        rec = np.empty((G, C, 2), f32)
        rec[..., 0] = np.where(nz[None, :], ystar, POISON)           # zero scale: the record does not hold row 0's value
        rec[..., 1] = arg.view(f32)
        c["rec"] = rec
    return c


def from_out(c):
    """The branch rule of include/pn2.h, in the kernels' float32: |gamma| >= (1 + |beta|) / 4 with gamma = scale / invstd."""
    ga = (c["scale"] / c["invstd"]).astype(f32)
    return np.abs(ga) >= f32(0.25) * (f32(1) + np.abs(c["beta"])), ga


def reduce_statement(c, rec=False):
    """fp64 statement and bounds of the reductions (module docstring): dict dZp (float32, exact), red0, red1, b0, b1 (per
    channel), branch (True: the `out` branch)."""
    mu, is_, be = c["mean"].astype(f64), c["invstd"].astype(f64), c["beta"].astype(f64)
    out = c["out"].astype(f64)
    on = c["out"] > 0
    dz = np.where(on, c["dOut"], f32(0))
    d = dz.astype(f64)
    y = c["ystar"].astype(f64)
    zs = c["scale"] == 0
    if rec:
        y = np.where(zs[None, :], c["rec_y"], y)
    xh = (y - mu) * is_
    n = c["G"]
    A0, A1 = np.abs(d).sum(0), np.abs(d * xh).sum(0)
    b0 = (n + 8) * U64 * A0
    acc = (n + 8) * U64 * A1
    b_gather = 3.01 * U32 * A1 + acc + b0
    fo, _ = from_out(c)
    if rec:
        fo = np.zeros_like(fo)
        e_y = scatter_ref.bound(c["C_in"], c["rec_abs"])           # [G, C]
        b_gather = b_gather + np.where(zs, 1.01 * is_ * (np.abs(d) * e_y).sum(0), 0.0)
    gam = np.where(fo, c["scale"].astype(f64) / is_, 1.0)
    b_out = 1.01 * U32 * (np.abs(d) * (A_OUT * np.abs(xh) + B_OUT * (np.abs(out) + np.abs(be)) / np.abs(gam))).sum(0) + acc + b0
    return dict(dZp=dz, red0=d.sum(0), red1=(d * xh).sum(0), b0=b0, b1=np.where(fo, b_out, b_gather), branch=fo, xhat=xh, live=on)


def emulate_reduce(c, mutant=None, rec=False):
    """pool_bwd_reduce_kernel / relu_bwd_reduce_kernel / pool_bwd_reduce_rec_kernel in numpy float32 with fp64 accumulation:
    returns (dZp with NaN where nothing was written, red0, red1).  Mutants: 1 the last group dropped, 2 group 0 counted
    twice, 3 row arg + 1 gathered, 4 the `out` branch without the division by gamma, 5 the mask taken as out >= 0."""
    G, K, C = c["G"], c["K"], c["C"]
    mu, is_, be = c["mean"], c["invstd"], c["beta"]
    fo, ga = from_out(c)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        rga = np.where(fo, f32(1) / ga, f32(0)).astype(f32)
        o, dzin = c["out"], c["dOut"]
        on = (o >= 0) if mutant == 5 else (o > 0)
        if rec:
            fo = np.zeros_like(fo)
            y = c["rec"][..., 0].copy()
            acc = np.broadcast_to(c["bias"][None, :], (G, C)).astype(f32)
            for j in range(c["C_in"]):
                acc = fma32(np.broadcast_to(c["W"][None, :, j], (G, C)), np.broadcast_to(c["x"][:, j:j + 1], (G, C)), acc)
            y = np.where((c["scale"] == 0)[None, :], acc, y)
        else:
            a = c["arg"].astype(np.int64) + (1 if mutant == 3 else 0)
            r = np.arange(G)[:, None] * K + a
            Yp = np.vstack([c["Y"], np.full((1, C), POISON, f32)])   # the row behind the last: whatever lies there
            y = Yp[np.minimum(r, G * K), np.broadcast_to(np.arange(C)[None, :], (G, C))]
        t_g = (dzin * (((y - mu).astype(f32) * is_).astype(f32))).astype(f32)
        ob = (o - be).astype(f32)
        t_o = (dzin * (ob if mutant == 4 else (ob * rga).astype(f32))).astype(f32)
        term = np.where(fo[None, :], t_o, t_g).astype(f64)
        dz = np.where(on, dzin, f32(0))
        w = np.ones(G)
        if mutant == 1:
            w[G - 1] = 0
        if mutant == 2:
            w[0] = 2
        red0 = (np.where(on, dzin.astype(f64), 0.0) * w[:, None]).sum(0)
        red1 = (np.where(on, term, 0.0) * w[:, None]).sum(0)
    if mutant == 1:
        dz = dz.copy()
        dz[G - 1] = np.nan
    return dz, red0, red1


# ================================================================================================ the two blocks, stand-alone

def stats_case(seed, P, C):
    """Sums of y and y^2 over P rows of C channels (fp64, drawn as moments so that every channel has a sound variance), with
    channel C // 2 made to CANCEL: sum y^2 / P - mean^2 = -1e-10 mean^2 < 0, which the clamp turns into invstd = 1 / sqrt(eps).
    gamma covers both signs and 0; running statistics to start from."""
    rng = np.random.default_rng(seed)
    m = rng.standard_normal(C) * 2.0
    v = rng.uniform(0.05, 3.0, C)
    s1, s2 = m * P, (v + m * m) * P
    cc = C // 2
    m_c = 3.0
    s1[cc], s2[cc] = m_c * P, m_c * m_c * P * (1.0 - 1e-10)
    gamma = rng.uniform(0.5, 1.5, C).astype(f32)
    gamma[1::5] *= -1
    gamma[3::7] = 0
    return dict(P=P, C=C, s1=s1, s2=s2, cancel=cc, gamma=gamma, beta=(rng.standard_normal(C) * 0.3).astype(f32),
                rmean=(rng.standard_normal(C) * 0.1).astype(f32), rvar=rng.uniform(0.5, 1.5, C).astype(f32),
                r0=rng.standard_normal(C) * P ** 0.5, r1=rng.standard_normal(C) * P ** 0.5)


def eval_block(gamma, beta, rmean, rvar, eps):
    """fp64 [4, C] affine block of eval-mode BatchNorm: the running statistics instead of the batch's."""
    invstd = 1.0 / np.sqrt(rvar.astype(f64) + eps)
    return np.stack([rmean.astype(f64), gamma.astype(f64) * invstd, beta.astype(f64), invstd])


# ================================================================================================ v1 / DenseCls relatives

def colsum_case(seed, G, rpg, C):
    """Operands of pn2_group_colsum (dZ, Y [G rpg, C], a coefficient block) with its fp64 statement s[g, c] = sum over the
    group's rows of c0 dz + q1 (y - mean) + q0 and the bound of an fp32 sum of rpg three-rounding terms."""
    rng = np.random.default_rng(seed)
    P = G * rpg
    dZ, Y = rng.standard_normal((P, C)).astype(f32), rng.standard_normal((P, C)).astype(f32)
    c0, q1 = (rng.standard_normal(C) * 0.5 + 1.0).astype(f32), (rng.standard_normal(C) * 0.05).astype(f32)
    q0, mu = (rng.standard_normal(C) * 0.05).astype(f32), (rng.standard_normal(C) * 0.3).astype(f32)
    t = [c0.astype(f64) * dZ, q1.astype(f64) * (Y.astype(f64) - mu), np.broadcast_to(q0.astype(f64), (P, C))]
    s = (t[0] + t[1] + t[2]).reshape(G, rpg, C).sum(1)
    A = (np.abs(t[0]) + np.abs(t[1]) + np.abs(t[2])).reshape(G, rpg, C).sum(1)
    return dict(G=G, rpg=rpg, C=C, dZ=dZ, Y=Y, coef=block(c0, q1, q0, mu), s=s, bound=scatter_ref.bound(rpg, A))


def noact_dense_case(seed, G, K, C):
    """Operands of pn2_bn_bwd_reduce_noact_dense: dDense [G K, C], dPool [G, C] (both multiples of 1/256, so the float32 sum dZ
    and red0 are exact), arg, Y, an affine block.  Statement: dZ = dDense + (k == arg) dPool; red0 = sum dZ (exact); red1 =
    sum dZ xhat within 3.01 u sum |dZ xhat| + the fp64 accumulation terms (the gather-branch count: y - mean, * invstd, * dz)."""
    rng = np.random.default_rng(seed)
    P = G * K
    dD = (rng.integers(-1024, 1025, (P, C)) / 256.0).astype(f32)
    dP = (rng.integers(-1024, 1025, (G, C)) / 256.0 + 8.0).astype(f32)                  # (+8: a pooled term nobody can miss)
    arg = rng.integers(0, K, (G, C)).astype(np.int32)
    Y = rng.standard_normal((P, C)).astype(f32)
    mean, invstd = (rng.standard_normal(C) * 0.3).astype(f32), rng.uniform(0.5, 2.0, C).astype(f32)
    hit = (np.arange(K)[None, :, None] == arg[:, None, :])
    dZ = (dD.reshape(G, K, C).astype(f64) + np.where(hit, dP[:, None, :].astype(f64), 0.0)).reshape(P, C)
    assert np.array_equal(dZ.astype(f32).astype(f64), dZ)
    xh = (Y.astype(f64) - mean) * invstd
    A0, A1 = np.abs(dZ).sum(0), np.abs(dZ * xh).sum(0)
    b0 = (P + 8) * U64 * A0
    return dict(G=G, K=K, C=C, dD=dD, dP=dP, arg=arg, Y=Y, aff=block(mean, np.ones(C, f32), np.zeros(C, f32), invstd), dZ=dZ.astype(f32),
                red0=dZ.sum(0), red1=(dZ * xh).sum(0), b0=b0, b1=3.01 * U32 * A1 + (P + 8) * U64 * A1 + b0)


# ================================================================================================ the case tables both tests walk

def reduce_cases():
    """(seed, G, K, C, C_in) of the pooled reductions: C in {1, 3, 13, 64, 67, 130} x (K in {1, 16, 33}) x (G in {1, 5, 17}),
    every other combination (each (K, G) pair with three of the C, each C with four or five pairs), and G = 16 * 1024 + 3:
    the second trip behind the 1024-workgroup cap (K = 1 keeps Y at 5 MB)."""
    out, pairs = [], [(K, G) for K in (1, 16, 33) for G in (1, 5, 17)]
    for i, C in enumerate((1, 3, 13, 64, 67, 130)):
        for j, (K, G) in enumerate(pairs):
            if (i + j) % 2 == 0:
                out.append((101 + 10 * i + j, G, K, C, (3, 64)[(i + j) // 2 % 2]))
    out.append((199, 16 * 1024 + 3, 1, 67, 3))
    return out


def dense_cases():
    """(seed, P, C) of pn2_relu_bwd_reduce: P in {1, 3, 63, 65} x C in {1, 5, 64, 65, 130} and P = 512 * 64 + 64 + 5 behind the
    512-workgroup cap (the second trip is a partial one: its later slots and the prefetch behind it run past P)."""
    out = [(201 + 5 * i + j, P, C) for i, P in enumerate((1, 3, 63, 65)) for j, C in enumerate((1, 5, 64, 65, 130))]
    out.append((299, 512 * 64 + 64 + 5, 65))
    return out


def relu_max_cap(cus, C):
    """Workgroup rows of pn2_bn_relu_max's bounded grid: 8 * CUs / gx, within [1, 65535]."""
    return max(1, min(65535, 8 * cus // lane_geometry(C)[2]))


def relu_max_cases(cus):
    """(form, seed, G, K, C) of pn2_bn_relu_max on a device of `cus` compute units; form in "k1" (K == 1), "wave" (one wave per
    group), "ksplit" (K >= 32 and G * gx <= 4096).  The lane geometries C in {1, 3, 4, 20, 64, 256, 260} (LPR 1, 1, 1, 8, 16,
    64, 64 x 2 column blocks) in every form's small cases; the grid-stride cases behind 4 * cap (* RPW) waves; K below RPW and
    K = RPW + 1 at C = 20 (RPW = 8); K = 32 with too many groups for ksplit; ksplit with G = cap + 1 (the barriers inside the
    second trip of the grid-stride loop)."""
    Cs = (1, 3, 4, 20, 64, 256, 260)
    out = [("k1", 300 + 2 * i + j, G, 1, C) for i, C in enumerate(Cs) for j, G in enumerate((1, 67))]
    out.append(("k1", 320, 4 * relu_max_cap(cus, 260) * lane_geometry(260)[1] + 5, 1, 260))
    n = 0
    for K in (2, 3, 16, 31):
        for G in (1, 5):
            out.append(("wave", 330 + n, G, K, Cs[n % 7]))
            out.append(("wave", 350 + n, G, K, Cs[(n + 3) % 7]))
            n += 1
    out += [("wave", 370, 5, 3, 20), ("wave", 371, 5, 9, 20), ("wave", 372, 4097, 32, 4), ("wave", 373, 4 * relu_max_cap(cus, 4) + 3, 2, 4)]
    n = 0
    for K in (32, 33, 35, 64, 127):
        for G in (1, 3):
            for C in (4, 64, 260):
                out.append(("ksplit", 400 + n, G, K, C))
                n += 1
    out += [("ksplit", 440 + i, relu_max_cap(cus, C) + 1, K, C) for i, (K, C) in enumerate(((33, 4), (127, 4), (32, 64), (35, 64), (32, 260)))]
    return out


def select_cases(cus):
    """(seed, G, C) of pn2_bn_pool_select (records drawn with rows below 64): C in {32, 96} x G in {1, 37} and, at C = 32, the
    first G past the bounded grid: more than 256 * 8 * CUs quads G C / 4 (65 541 groups on 256 compute units)."""
    return [(501, 1, 32), (537, 37, 32), (502, 1, 96), (538, 37, 96), (599, 256 * cus + 5, 32)]


def relu_max_form(cus, G, K, C):
    """The form pn2_bn_relu_max takes (the host-side rule of the issue / csrc/mlp.hip), with the number of trips its busiest
    workgroup row makes through the grid-stride loop."""
    _, rpw, gx = lane_geometry(C)
    cap = relu_max_cap(cus, C)
    if K >= 32 and G * gx <= 4096 and G <= 65535:
        return "ksplit", -(-G // min(G, cap))
    waves = -(-G // rpw) if K == 1 else G
    gy = min(-(-waves // 4), cap)
    return ("k1" if K == 1 else "wave"), -(-waves // (4 * gy))
