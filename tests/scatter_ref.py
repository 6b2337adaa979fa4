"""fp64 statements of the index-driven kernels (csrc/gather.hip, csrc/scatter.hip, the factorised first layer of
csrc/grouped.hip), the a-priori error bound their scattered sums are held to, and the index / data generators of
tests/test_scatter_gpu.py.  A test helper written from the formulas of include/pn2.h, for clarity, not speed; every
function takes tensors of any device and answers on that device.

THE BOUND.  An fp32 sum of n terms, added in ANY order, each term carrying at most k roundings of its own, differs from
the exact sum by at most (n - 1 + k) u A / (1 - (n - 1 + k) u), u = 2^-24, A = the sum of the terms' absolute values
(Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  ``bound(n, A)`` = 1.05 (n + 4) u A covers k <= 3
(dY = fma(c0, dZ, fma(q1, y - mean, q0)): three roundings; w * g: one), the denominator for n < 5e5 and the fp64
rounding of A.  An output element that no term lands on (n == 0) must be exactly 0.

EXACTLY SUMMABLE DATA.  The bound grows like n against a signal (one missing member) of A / n, so it goes blind on long
segments.  The ``exact_*`` generators draw every factor from a binary grid so that every term is a multiple of one
``unit`` and A / unit < 2^24 for every output element (``assert_exactly_summable``): every partial sum in every order is
then an fp32 number, and a kernel's output must be BIT-equal to the fp64 sum cast to float32 whatever its chunking,
atomics' order or replica folding.
"""
import numpy as np
import torch

U32 = 2.0 ** -24                     # unit roundoff of float32


def bound(n, A):
    """Per-element tolerance of an fp32 sum of n terms with sum of absolute values A (see the module docstring)."""
    return 1.05 * (n + 4) * U32 * A


def assert_exactly_summable(A, unit):
    assert float(A.max()) / unit < 2 ** 24, (float(A.max()) / unit, unit)


# ------------------------------------------------------------------------------------------------ forward statements

def interp_fwd(points2, idx, w):
    """points2 [B,S,D] f32, idx [B,N,3], w [B,N,3] f32 -> [B,N,D] f32 = ((p0*w0 + p1*w1) + p2*w2), every operation a
    float32 operation rounded on its own (separate tensor operations: nothing is fused)."""
    assert points2.dtype == torch.float32 and w.dtype == torch.float32
    B, S, D = points2.shape
    N = idx.shape[1]
    rows = (idx + torch.arange(B, device=idx.device).view(B, 1, 1) * S).reshape(-1)
    p = points2.reshape(B * S, D)[rows].view(B, N, 3, D)
    t0 = torch.mul(p[:, :, 0], w[:, :, 0:1])
    t1 = torch.mul(p[:, :, 1], w[:, :, 1:2])
    t2 = torch.mul(p[:, :, 2], w[:, :, 2:3])
    return torch.add(torch.add(t0, t1), t2)


def _centred(xyz, new_xyz, idx):
    """(xyz[b, idx[b,s,k]] - new_xyz[b,s]) in fp64 [B,S,K,3], and the in-range mask [B,S,K]."""
    B, N, _ = xyz.shape
    valid = (idx >= 0) & (idx < N)
    j = torch.where(valid, idx, torch.zeros_like(idx))
    rows = (j + torch.arange(B, device=idx.device).view(B, 1, 1) * N).reshape(-1)
    q = xyz.double().reshape(B * N, 3)[rows].view(idx.shape + (3,))
    return q - new_xyz.double().unsqueeze(2), valid, rows


def group_affine_fwd(Zf, xyz, new_xyz, idx, Wx):
    """Zf [B*N, C] , xyz [B,N,3], new_xyz [B,S,3], idx [B,S,K] in range, Wx [C,3] ->
    (Y [P,C] fp64 = Zf[idx] + Wx (xyz[idx] - centre), mag [P,C] = |z| + sum_a |Wx_a d_a|, sum y [C], sum y^2 [C])."""
    d, valid, rows = _centred(xyz, new_xyz, idx)
    assert bool(valid.all())
    d = d.reshape(-1, 3)
    z = Zf.double()[rows]
    W = Wx.double()
    Y = z + d @ W.t()
    mag = z.abs() + d.abs() @ W.abs().t()
    return Y, mag, Y.sum(0), (Y * Y).sum(0)


# ----------------------------------------------------------------------------------------------- backward statements

def scatter_sum(idx, terms, T, absterms=None):
    """idx [B,M] int64, terms [B,M,D] fp64 -> (sum [B,T,D] fp64 with out[b, idx[b,m]] += terms[b,m], n [B,T] the number
    of terms per target, A [B,T,D] the sum of their absolute values).  Entries outside [0, T) are dropped."""
    B, M = idx.shape
    D = terms.shape[2]
    valid = (idx >= 0) & (idx < T)
    rows = (torch.where(valid, idx, torch.zeros_like(idx)) + torch.arange(B, device=idx.device).view(B, 1) * T).reshape(-1)
    keep = valid.reshape(-1, 1).double()
    t = terms.reshape(B * M, D).double() * keep
    a = (terms.abs() if absterms is None else absterms).reshape(B * M, D).double() * keep
    # a few targets with very many members (one owner for a whole cloud): member m adds into copy m % copies of its target
    # and the copies are summed afterwards -- the same fp64 sum without a long queue of additions on one address
    copies = 64 if B * M > 64 * B * T else 1
    rows = rows * copies + torch.arange(B * M, device=idx.device) % copies
    acc = torch.zeros(B * T * copies, 2 * D + 1, dtype=torch.float64, device=idx.device)
    acc.index_add_(0, rows, torch.cat([t, a, keep], 1))
    acc = acc.view(B, T, copies, 2 * D + 1).sum(2)
    return acc[:, :, :D], acc[:, :, 2 * D], acc[:, :, D:2 * D]


def interp_bwd(grad_out, col0, D, idx, w, S):
    """grad_out [B,N,ld], idx [B,N,3], w [B,N,3] -> dP2[b, idx[b,n,k], :] += w[b,n,k] grad_out[b,n,col0:col0+D]."""
    B, N, _ = idx.shape
    g = grad_out[:, :, col0:col0 + D].double()
    terms = (w.double().unsqueeze(3) * g.unsqueeze(2)).reshape(B, 3 * N, D)
    return scatter_sum(idx.reshape(B, 3 * N), terms, S)


def gather_rows_bwd(grad_out, idx, N):
    """grad_out [B,M,C], idx [B,M] -> grad_points[b, idx[b,m], :] += grad_out[b,m,:]."""
    return scatter_sum(idx, grad_out.double(), N)


def group_bwd(grad_rows, idx, B, N, S, K, D, xyz_first):
    """grad_rows [B*S*K, ld] -> grad_points[b, idx[b,s,k], :] += the D feature columns of row (b,s,k); idx None: k."""
    c = 3 if xyz_first else 0
    if idx is None:
        idx = torch.arange(K, device=grad_rows.device).expand(B, S, K)
    return scatter_sum(idx.reshape(B, S * K), grad_rows[:, c:c + D].double().reshape(B, S * K, D), N)


def group_affine_bwd(dZ, Y, coef, xyz, new_xyz, idx):
    """dZ, Y [P,C]; coef = (c0, q1, q0, mean) each [C]; idx [B,S,K] -> (dY [P,C], G [B,N,C], n [B,N], A [B,N,C],
    dWx [C,3], AW [C,3]) with dY = c0 dZ + q1 (y - mean) + q0, G = scatter of dY, dWx = dY^T (xyz[idx] - centre); a
    term's absolute value is |c0 dZ| + |q1 (y - mean)| + |q0| (A: summed per target; AW: times |xyz[idx] - centre|,
    summed over all rows).  Out-of-range entries contribute nothing anywhere."""
    B, N, _ = xyz.shape
    S, K = idx.shape[1:]
    c0, q1, q0, mu = (c.double() for c in coef)
    t0, t1 = c0 * dZ.double(), q1 * (Y.double() - mu)
    dY = t0 + t1 + q0
    absdY = t0.abs() + t1.abs() + q0.abs()
    d, valid, _ = _centred(xyz, new_xyz, idx)
    C = dY.shape[1]
    G, n, A = scatter_sum(idx.reshape(B, S * K), dY.view(B, S * K, C), N, absdY.view(B, S * K, C))
    keep = valid.reshape(-1, 1).double()
    dWx = (dY * keep).t() @ d.reshape(-1, 3)
    AW = (absdY * keep).t() @ d.reshape(-1, 3).abs()
    return dY, G, n, A, dWx, AW


# ------------------------------------------------------------------------------------------------- index generators
# Each returns int64 [B, M] with values in [0, T) (unless it says otherwise), different per cloud.  M members onto T
# targets: the interpolation's idx [B,N,3] is the [B, 3N] view (T = S), the grouping's idx [B,S,K] the [B, S*K] view
# (T = N).  "Segment" = the members of one target, consecutive in the target-sorted member list of pn2_invert_index.

def segments_index(B, M, T, length, seed):
    """Every segment exactly `length` members long (the last one M % length if that is not 0), segment i of the sorted
    list starting at member i * length; the ceil(M / length) owning targets are a random ascending subset of [0, T)
    (all others are empty), and the positions are randomly permuted."""
    nseg = -(-M // length)
    assert nseg <= T
    rng = np.random.default_rng(seed)
    idx = np.empty((B, M), np.int64)
    for b in range(B):
        targets = np.sort(rng.choice(T, nseg, replace=False))
        idx[b, rng.permutation(M)] = targets[np.arange(M) // length]
    return torch.from_numpy(idx)


def random_index(B, M, T, seed):
    """Uniformly random targets (T = 3: three targets only; T >> M: most targets empty)."""
    return torch.from_numpy(np.random.default_rng(seed).integers(0, T, (B, M)))


def with_dropped(idx, T, seed, fraction=0.1):
    """A copy with `fraction` of the entries out of range (-1 and T + 5 alternating): dropped by the segmented path."""
    rng = np.random.default_rng(seed)
    out = idx.clone().numpy()
    for b in range(out.shape[0]):
        pos = rng.choice(out.shape[1], max(1, int(out.shape[1] * fraction)), replace=False)
        out[b, pos[0::2]] = -1
        out[b, pos[1::2]] = T + 5
    return torch.from_numpy(out)


def segment_lengths(idx, T):
    """[B, T] member count of every target (out-of-range entries not counted)."""
    B = idx.shape[0]
    out = np.zeros((B, T), np.int64)
    a = idx.numpy()
    for b in range(B):
        v = a[b][(a[b] >= 0) & (a[b] < T)]
        out[b] = np.bincount(v, minlength=T)
    return out


CHUNKS = (16, 32, 64)                 # the member counts per lane group seg_chunk() of csrc/scatter.hip chooses from


def constructed_cases(M, seed, B=3):
    """[(name, idx [B,M], T)]: the boundary cases of the store-versus-atomic rule for EVERY chunk length (each case is
    run with each forced chunk, so a segment length of 32 is "exactly a chunk", "two chunks" and "half a chunk")."""
    cases = []
    for length in sorted({c + d for c in CHUNKS for d in (-1, 0, 1)} | {1}):
        T = -(-M // length) + 7
        cases.append(("len%d" % length, segments_index(B, M, T, length, seed + length), T))
    cases.append(("one_owner", segments_index(B, M, 5, M, seed + 1000), 5))            # one segment over many chunks
    cases.append(("three_targets", random_index(B, M, 3, seed + 1001), 3))
    cases.append(("mostly_empty", random_index(B, M, 3 * M + 11, seed + 1002), 3 * M + 11))
    return cases


# -------------------------------------------------------------------------------------------------- data generators

def random_interp_data(B, N, ld, seed, device="cpu"):
    """(grad_out [B,N,ld] ~ N(0,1), w [B,N,3] positive, rows summing to 1 like the inverse-distance weights)."""
    g = torch.Generator(device=device).manual_seed(seed)
    w = torch.rand(B, N, 3, generator=g, device=device) + 1e-3
    return torch.randn(B, N, ld, generator=g, device=device), (w / w.sum(-1, keepdim=True)).float()


def exact_interp_data(B, N, ld, seed, device="cpu"):
    """Integers in [-8, 8] and weights in {1, 1/2, 1/4}: every term a multiple of unit = 1/4, |term| <= 8."""
    g = torch.Generator(device=device).manual_seed(seed)
    grad = torch.randint(-8, 9, (B, N, ld), generator=g, device=device).float()
    w = torch.tensor([1.0, 0.5, 0.25], device=device)[torch.randint(0, 3, (B, N, 3), generator=g, device=device)]
    return grad, w


EXACT_INTERP_UNIT = 0.25


def random_affine_data(B, N, S, K, C, seed, device="cpu"):
    """(dZ [P,C], Y [P,C], coef (c0, q1, q0, mean), xyz [B,N,3], new_xyz [B,S,3]) in the ranges of a BatchNorm backward:
    c0 ~ 1, q1 and q0 ~ 1e-3 (tests/test_mlp_gpu.py's fixed-operand cases use the same)."""
    g = torch.Generator(device=device).manual_seed(seed)
    P = B * S * K
    rn = lambda *shape: torch.randn(*shape, generator=g, device=device)
    coef = (rn(C) * 0.5 + 1.0, rn(C) * 1e-3, rn(C) * 1e-3, rn(C) * 0.3)
    return (rn(P, C), rn(P, C) * 1.5 + 0.3, coef, torch.rand(B, N, 3, generator=g, device=device) * 2 - 1,
            torch.rand(B, S, 3, generator=g, device=device) * 2 - 1)


def exact_affine_data(B, N, S, K, C, seed, device="cpu"):
    """dZ in {-1, 0, 1}, c0 in {1, 1/2}, y and mean in {-1/2, 0, 1/2}, q1 in {1/4, -1/4}, q0 in {-1/8, 0, 1/8}: dY is a
    multiple of 1/8 with |c0 dZ| + |q1 (y - mean)| + |q0| <= 1.375 (11 units); coordinates in {0, 1/2}: the centred
    difference is a multiple of 1/2, |.| <= 1/2, so a dWx term is a multiple of 1/16 and at most 11 units."""
    g = torch.Generator(device=device).manual_seed(seed)
    P = B * S * K
    pick = lambda vals, *shape: torch.tensor(vals, device=device)[torch.randint(0, len(vals), shape, generator=g, device=device)]
    coef = (pick([1.0, 0.5], C), pick([0.25, -0.25], C), pick([-0.125, 0.0, 0.125], C), pick([-0.5, 0.0, 0.5], C))
    return (pick([-1.0, 0.0, 1.0], P, C), pick([-0.5, 0.0, 0.5], P, C), coef,
            pick([0.0, 0.5], B, N, 3), pick([0.0, 0.5], B, S, 3))


EXACT_AFFINE_UNIT_G = 0.125
EXACT_AFFINE_UNIT_DWX = 0.0625


# -------------------------------------------------------------------------- float32 sums in three orders (CPU tests)

def f32_sums_three_orders(terms):
    """terms: float32 numpy [n, D] -> the column sums accumulated in float32 sequentially, reversed and pairwise."""
    terms = np.ascontiguousarray(terms, np.float32)
    seq = np.zeros(terms.shape[1], np.float32)
    for row in terms:
        seq = (seq + row).astype(np.float32)
    rev = np.zeros(terms.shape[1], np.float32)
    for row in terms[::-1]:
        rev = (rev + row).astype(np.float32)
    level = terms
    while level.shape[0] > 1:
        if level.shape[0] % 2:
            level = np.concatenate([level, np.zeros((1, level.shape[1]), np.float32)])
        level = (level[0::2] + level[1::2]).astype(np.float32)
    pair = level[0] if level.shape[0] else np.zeros(terms.shape[1], np.float32)
    return seq, rev, pair
