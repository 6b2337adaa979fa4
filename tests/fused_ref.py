"""Fixed operands and fp64 statements of the two kernels that do several jobs in one launch: pn2_group_conv_fwd
(csrc/grouped.hip: gather + centre + concat + the first conv + the BatchNorm sums) and pn2_fused_eval (csrc/eval.hip:
gather -> up to four linear + ReLU layers -> max over the neighbours).  A test helper written from the formulas of
include/pn2.h, for clarity, not speed; every function takes tensors of any device and answers on that device.

NO DECISION IN THE PATH.  xyz, centres, features, the neighbour index, fp32 weights and biases are drawn directly; the
weights of pn2_fused_eval are drawn as the folded W', b' themselves.  No BatchNorm fold, no ball query, no FPS.

GROUPED ROWS (``grouped_rows``) are stated as separately rounded float32: the centred columns are fp32(xyz_j - c_s), ONE
rounding (a single torch.sub), the features are copies, the columns [3 + D, ldx) are zero.  X of pn2_group_conv_fwd must
be bit-equal to that.

THE CHAIN (``chain64``) is evaluated in fp64 from the EXACT centred difference, ReLU between the layers; with pool > 0 the
max over the group is taken before the last ReLU (relu(max) = max(relu)).

THE RUNNING BOUND, derived, not fitted.  u = 2^-24.  An fp32 dot product of K terms plus a bias, accumulated in any order
(MFMA partial sums included), then rounded once more when it is stored, differs from the exact one by at most
gamma_{K+2} (|W| |a| + |b|), gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, section
3.1); 1.05 covers the denominator for n < 4e5 and the second-order term of evaluating it on the exact a.  An error E in
the layer's input moves the output by at most |W| E.  So per element
    E_0 = u |x| on the three centred columns (the one rounding of the subtraction), 0 elsewhere,
    E_l = |W_l| E_{l-1} + 1.05 (K_l + 2) u (|W_l| |a_{l-1}| + |b_l|),
ReLU and max are 1-Lipschitz, and the bound of a pooled output is the max of E over its group.  It is stated on the
CENTRED magnitudes: at KITTI scale (coordinates ~70, differences ~1e-3: ``kitti=True``) a kernel that multiplies before
it subtracts is off by u * 70 |W|, five orders above it.

THE INDEX of every cloud contains 0, N - 1 and duplicates (one adjacent, one far away); B >= 2 in every case, so the
b * N offset is live.

THE CASES of tests/test_group_conv_gpu.py and tests/test_fused_eval_gpu.py are listed here (GROUP_CONV_K, GROUP_CONV_CD,
EVAL_CASES) together with the functions that state their tolerances (group_conv_errors / group_conv_ok, eval_errors /
eval_ok), so that tests/test_fused_ref_cpu.py evaluates the same formulas against the same assertions without a GPU.
"""
import torch

from mlp_ref import SENTINEL, STAT_REPLICAS, check_guards, guarded, rel, round4  # noqa: F401  (re-exported for the tests)
from scatter_ref import U32

POISON = 1e30                        # behind the columns a kernel may read: large, finite, visible in any sum


def round8(c):
    return (c + 7) & ~7


def _gen(dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return g, (lambda *s: torch.randn(*s, device=dev, generator=g)), (lambda *s: torch.rand(*s, device=dev, generator=g))


# ------------------------------------------------------------------------------------------------ operands

def draw_geometry(dev, B, N, S, K, D, seed, kitti=False, group_all=False):
    """xyz [B,N,3], points [B,N,D] (None for D == 0), new_xyz [B,S,3], idx [B,S,K] int64.  kitti: clouds and centres at
    offsets of about 70 with differences of about 1e-3 and features of that size; otherwise both uniform in [-1, 1] and
    features ~ N(0, 1).  group_all: S == 1, K == N, new_xyz and idx are None (the rows are the cloud in order, un-centred)."""
    assert B >= 2 and S * K >= 6
    g, randn, rand = _gen(dev, seed)
    if kitti:
        off = torch.tensor([70.0, -68.5, 71.25], device=dev)
        xyz = off + (rand(B, N, 3) * 2 - 1) * 1e-3
        new_xyz = off + (rand(B, S, 3) * 2 - 1) * 1e-3
    else:
        xyz, new_xyz = rand(B, N, 3) * 2 - 1, rand(B, S, 3) * 2 - 1
    points = randn(B, N, D) * (1e-3 if kitti else 1.0) if D else None      # (kitti: features at the centred scale, so the bound stays there)
    if group_all:
        assert S == 1 and K == N
        return dict(xyz=xyz, points=points, new_xyz=None, idx=None, B=B, N=N, S=S, K=K, D=D)
    idx = torch.randint(0, N, (B, S * K), device=dev, generator=g)
    idx[:, 0] = 0
    idx[:, -1] = N - 1
    idx[:, 2] = idx[:, 1]
    idx[:, (S * K) // 2] = idx[:, 1]
    return dict(xyz=xyz.contiguous(), points=points, new_xyz=new_xyz.contiguous(), idx=idx.view(B, S, K).contiguous(), B=B, N=N, S=S,
                K=K, D=D)


def draw_weight(randn, co, ci, ldw, scale, pad_to=None):
    """W [co, ci] * scale inside a [co, ldw] storage: zero in the columns [ci, pad_to) (what the kernel may read: pad_to =
    round8(ci) for pn2_fused_eval, ci for pn2_group_conv_fwd), POISON behind them.  Returns (view [co, ci], storage)."""
    pad_to = ci if pad_to is None else pad_to
    assert ldw >= pad_to
    store = torch.zeros(co, ldw, device=randn(1).device)
    store[:, :ci] = randn(co, ci) * scale
    store[:, pad_to:] = POISON
    return store[:, :ci], store


def draw_layers(dev, K0, widths, seed, ldw_extra=0, dead=None):
    """The folded layers of one pn2_fused_eval chain K0 -> widths[0] -> ...: [(W view [N, K], bias [N], storage [N, ldw],
    ldw)], ldw = round8(K) + ldw_extra, weights ~ N(0, 2 / K), biases ~ 0.1 N(0, 1).  dead: that channel of the LAST layer
    gets the bias -1000, so that every one of its pre-activations is below zero."""
    _, randn, _ = _gen(dev, seed)
    layers, K = [], K0
    for l, n in enumerate(widths):
        ldw = round8(K) + ldw_extra
        W, store = draw_weight(randn, n, K, ldw, (2.0 / K) ** 0.5, round8(K))
        b = randn(n) * 0.1
        if dead is not None and l == len(widths) - 1:
            b[dead] = -1000.0
        layers.append((W, b, store, ldw))
        K = n
    return layers


# ------------------------------------------------------------------------------------------------ grouped rows

def grouped_rows(geo, xyz_first, ldx):
    """-> (X [P, ldx] float32 as stated in the module docstring, x64 [P, 3 + D] the same rows with the EXACT centred
    difference in fp64, E0 [P, 3 + D] = u |x| on the centred columns, 0 elsewhere)."""
    xyz, points, new_xyz, idx = geo["xyz"], geo["points"], geo["new_xyz"], geo["idx"]
    B, N, S, K, D = geo["B"], geo["N"], geo["S"], geo["K"], geo["D"]
    dev = xyz.device
    if idx is None:
        idx = torch.arange(K, device=dev).expand(B, S, K)
    rows = (idx + torch.arange(B, device=dev).view(B, 1, 1) * N).reshape(-1)
    q = xyz.reshape(B * N, 3)[rows]
    P = B * S * K
    if new_xyz is not None:
        c = new_xyz.reshape(B * S, 1, 3).expand(B * S, K, 3).reshape(P, 3)
        c32, c64 = torch.sub(q, c), q.double() - c.double()
        e0 = U32 * c64.abs()
    else:
        c32, c64, e0 = q, q.double(), torch.zeros(P, 3, dtype=torch.float64, device=dev)
    xo, fo = (0, 3) if xyz_first else (D, 0)
    X = torch.zeros(P, ldx, device=dev)
    x64 = torch.zeros(P, 3 + D, dtype=torch.float64, device=dev)
    E0 = torch.zeros_like(x64)
    X[:, xo:xo + 3], x64[:, xo:xo + 3], E0[:, xo:xo + 3] = c32, c64, e0
    if D:
        f = points.reshape(B * N, D)[rows]
        X[:, fo:fo + D], x64[:, fo:fo + D] = f, f.double()
    return X, x64, E0


# ------------------------------------------------------------------------------------------------ the chain

def chain64(x64, E0, layers, pool):
    """fp64 chain and its running bound (module docstring).  layers: [(W [N, K], b [N], ...)].  -> (out, bound), both
    [P, N_L] (pool == 0) or [P / pool, N_L]."""
    a, E = x64, E0
    for l, layer in enumerate(layers):
        W, b = layer[0].double(), layer[1].double()
        K = W.shape[1]
        z = a @ W.t() + b
        E = E @ W.abs().t() + 1.05 * (K + 2) * U32 * (a.abs() @ W.abs().t() + b.abs())
        if l + 1 < len(layers):
            a = torch.relu(z)
    if pool:
        z, E = z.view(-1, pool, z.shape[1]).amax(1), E.view(-1, pool, E.shape[1]).amax(1)
    return torch.relu(z), E


def chain32(X, layers, pool):
    """The same chain in plain torch float32 on the float32 rows X [P, >= K0] -- the evaluation whose own error against fp64
    (e32) the 4x rule of tests/test_fused_eval_gpu.py is measured with.  Never a kernel of this library."""
    a = X[:, :layers[0][0].shape[1]]
    for l, layer in enumerate(layers):
        z = a @ layer[0].t() + layer[1]
        if l + 1 < len(layers):
            a = torch.relu(z)
    if pool:
        z = z.view(-1, pool, z.shape[1]).amax(1)
    return torch.relu(z)


# ------------------------------------------------------------------------------------------------ pn2_group_conv_fwd

# The neighbour counts and the C_out x D grid of the GPU file; layout and pitches are crossed there.  K = 3 and 96 do not
# divide 64: a slab straddles groups (and clouds).
GROUP_CONV_K = (16, 32, 64, 3, 96)
GROUP_CONV_CD = [(co, D) for co in (32, 64) for D in (1, 3, 6, 9)]


def group_conv_case(dev, B, S, K, D, co, seed, N=257, kitti=False, ldw_extra=0):
    """Operands of one pn2_group_conv_fwd problem (without the layout choices xyz_first / ldx / ldy, which
    ``group_conv_statement`` takes): geometry, W [co, 3 + D] at pitch 3 + D + ldw_extra, bias."""
    geo = draw_geometry(dev, B, N, S, K, D, seed, kitti)
    _, randn, _ = _gen(dev, seed + 1)
    ci = 3 + D
    W, store = draw_weight(randn, co, ci, ci + ldw_extra, 0.5)
    return dict(geo=geo, W=W, w_store=store, ldw=ci + ldw_extra, bias=randn(co) * 0.1, co=co)


def group_conv_statement(case, xyz_first, ldx):
    """-> dict(X float32 [P, ldx] (bit-exact statement), Y fp64 [P, co], bound [P, co], s1 = sum y, s2 = sum y^2, sabs = sum |y|)."""
    X, x64, E0 = grouped_rows(case["geo"], xyz_first, ldx)
    W, b = case["W"].double(), case["bias"].double()
    K = W.shape[1]
    Y = x64 @ W.t() + b
    bound = E0 @ W.abs().t() + 1.05 * (K + 2) * U32 * (x64.abs() @ W.abs().t() + b.abs())
    return dict(X=X, Y=Y, bound=bound, s1=Y.sum(0), s2=(Y * Y).sum(0), sabs=Y.abs().sum(0))


def group_conv_errors(st, X, Y, sums):
    """What a result (X [P, ldx] float32, Y [P, co] float32, sums [2, co] fp64 or None) misses of the statement `st`, as a
    tensor of five numbers on the device (no synchronisation): elements of X that are not bit-equal, elements of Y outside
    the bound (a NaN is outside), worst |err| / bound, worst error of sum y relative to sum |y| and of sum y^2 relative to
    sum y^2.  ``group_conv_ok`` states the tolerances."""
    xd = (X.contiguous().view(torch.int32) != st["X"].view(torch.int32)).sum().double()
    err = (Y.double() - st["Y"]).abs()
    outside = (~(err <= st["bound"])).sum().double()
    ratio = (err / st["bound"]).max()
    if sums is None:
        e1 = e2 = torch.zeros((), dtype=torch.float64, device=Y.device)
    else:
        e1 = ((sums[0] - st["s1"]).abs() / st["sabs"]).max()
        e2 = ((sums[1] - st["s2"]).abs() / st["s2"]).max()
    return torch.stack([xd, outside, ratio, e1, e2])


STAT_TOL = 1e-5                      # the bound tests/test_mlp_seams_gpu.py holds the same sums to


def group_conv_ok(e):
    """e: the five numbers of ``group_conv_errors`` (on the host).  X bit-equal, Y inside the bound, sums within STAT_TOL."""
    return e[0] == 0 and e[1] == 0 and e[3] <= STAT_TOL and e[4] <= STAT_TOL


# ------------------------------------------------------------------------------------------------ pn2_fused_eval

# Grouped cases: B, N, S, Knb (= pool), D, xyz_first, widths; optional kitti, ldw_extra, dead (a dead last-layer channel),
# group_all.  Plain-row cases ("rows": X given): P, K0, ldx, widths, pool.  What each one reaches is tabulated in the
# docstring of tests/test_fused_eval_gpu.py.
EVAL_CASES = {
    # ---- grouped
    "g16_k3_13":        dict(B=3, N=200, S=3, Knb=16, D=0, xyz_first=1, widths=[13]),
    "g16_kitti_40_520": dict(B=3, N=150, S=5, Knb=16, D=9, xyz_first=0, widths=[40, 520], kitti=True),
    "g32_k4_33_33":     dict(B=2, N=120, S=5, Knb=32, D=1, xyz_first=0, widths=[33, 33], dead=7),
    "g32_kitti_32_33":  dict(B=2, N=120, S=3, Knb=32, D=0, xyz_first=1, widths=[32, 33], kitti=True),
    "g64_k9_32_40_160": dict(B=2, N=300, S=3, Knb=64, D=6, xyz_first=0, widths=[32, 40, 160], ldw_extra=8, dead=33),
    "g96_k12_8_13_33_520": dict(B=2, N=250, S=2, Knb=96, D=9, xyz_first=1, widths=[8, 13, 33, 520]),
    "g128_k16_kitti_40_13": dict(B=2, N=300, S=2, Knb=128, D=13, xyz_first=0, widths=[40, 13], kitti=True, ldw_extra=4),
    "group_all_33_160": dict(B=2, N=64, S=1, Knb=64, D=6, xyz_first=1, widths=[33, 160], group_all=True),
    # ---- plain rows
    "rows1_12_40_13":   dict(rows=1, K0=12, ldx=12, widths=[40, 13], pool=0),
    "rows31_12_40_13":  dict(rows=31, K0=12, ldx=16, widths=[40, 13], pool=0),
    "rows32_12_40_13":  dict(rows=32, K0=12, ldx=12, widths=[40, 13], pool=0),
    "rows33_12_40_13":  dict(rows=33, K0=12, ldx=12, widths=[40, 13], pool=0),
    "rows95_16_33_160": dict(rows=95, K0=16, ldx=20, widths=[33, 160], pool=0, ldw_extra=8),
    "rows33_deep_wide": dict(rows=33, K0=520, ldx=520, widths=[256, 128, 13], pool=0),
    "rows96_pool32_32_8_33": dict(rows=96, K0=32, ldx=36, widths=[8, 33], pool=32),
}


def eval_case(dev, name, spec=None):
    """Operands and fp64 statement of one EVAL_CASES entry (or of `spec`): dict with X (float32 rows: the plain input, or
    the stated grouped rows), geo (None for plain rows), layers, pool, P, ref, bound, e32 (module docstring / chain32)."""
    c = dict(EVAL_CASES[name] if spec is None else spec)
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100003
    if "rows" in c:
        P, K0, pool = c["rows"], c["K0"], c["pool"]
        _, randn, _ = _gen(dev, seed)
        X = torch.full((P, c["ldx"]), POISON, device=dev)
        X[:, :K0] = randn(P, K0)
        x64, E0, geo = X[:, :K0].double(), torch.zeros(P, K0, dtype=torch.float64, device=dev), None
    else:
        geo = draw_geometry(dev, c["B"], c["N"], c["S"], c["Knb"], c["D"], seed, c.get("kitti", False), c.get("group_all", False))
        K0, pool, P = 3 + c["D"], c["Knb"], c["B"] * c["S"] * c["Knb"]
        X, x64, E0 = grouped_rows(geo, c["xyz_first"], round4(K0))
    layers = draw_layers(dev, K0, c["widths"], seed + 1, c.get("ldw_extra", 0), c.get("dead"))
    ref, bound = chain64(x64, E0, layers, pool)
    e32 = float((chain32(X, layers, pool).double() - ref).abs().max())
    return dict(c, name=name, X=X, geo=geo, layers=layers, pool=pool, P=P, K0=K0, ref=ref, bound=bound, e32=e32,
                refmax=float(ref.abs().max()))


def eval_errors(st, out):
    """What `out` (float32, the shape of st["ref"]) misses of the statement, as three numbers on the device: elements
    outside the running bound (a NaN is outside), worst |err| / bound, max |err|."""
    err = (out.double() - st["ref"]).abs()
    return torch.stack([(~(err <= st["bound"])).sum().double(), (err / st["bound"]).max(), err.max()])


def eval_ok(st, e):
    """e: the numbers of ``eval_errors`` on the host.  Every element inside the running bound AND max |err| <= max(4 e32,
    4 u max|ref|), e32 the error of plain torch float32 on the same operands: the 4x rule of tests/test_mlp_gpu.py."""
    return e[0] == 0 and e[2] <= max(4.0 * st["e32"], 4.0 * U32 * st["refmax"])
