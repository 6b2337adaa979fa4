"""fp64 restatement of the one-directional Chamfer distance, written from its formulas in this project's own words: a test
helper, not a port.

    d[b,n]   = min_m || p1[b,n,:] - p2[b,m,:] ||_2          arg-min m*[b,n]: the LOWEST m on equal distance
    value    = (1/B) sum_b sum_n d[b,n]
    dp1[b,n] = (g/B) (p1[b,n] - p2[b,m*]) / d[b,n], a zero row where d == 0
    dp2[b,m] = - sum_{n : m*(n) = m} dp1[b,n]

Everything is evaluated in row chunks, so nothing larger than ``budget`` bytes is ever held (a 65 536 x 65 536 fp64 matrix would
be 34 GB).  ``stock_chamfer`` is the formulation the HIP kernels replace (broadcast difference -> norm -> min -> sum in
stock fp32 torch with autograd): tools/bench_chamfer.py and the speed test time it.
"""
import numpy as np
import torch


def _rows_per_chunk(B, M, D, budget):
    return max(1, int(budget // (8 * B * M * (D + 2))))


def nearest(p1, p2, budget=1 << 28):
    """p1 [B,N,D], p2 [B,M,D] (any float dtype, any device) -> (d [B,N] fp64, idx [B,N] int64), lowest index on ties."""
    p1, p2 = p1.double(), p2.double()
    B, N, D = p1.shape
    M = p2.shape[1]
    d = torch.empty(B, N, dtype=torch.float64, device=p1.device)
    idx = torch.empty(B, N, dtype=torch.int64, device=p1.device)
    order = torch.arange(M, device=p1.device)
    step = _rows_per_chunk(B, M, D, budget)
    for r in range(0, N, step):
        diff = p1[:, r:r + step, None, :] - p2[:, None, :, :]
        d2 = (diff * diff).sum(-1)                                    # [B, rows, M]
        lo = d2.min(dim=2, keepdim=True)[0]
        idx[:, r:r + step] = torch.where(d2 == lo, order, M).min(dim=2)[0]
        d[:, r:r + step] = lo[:, :, 0].sqrt()
    return d, idx


def nearest_gap(p1, p2, budget=1 << 28):
    """Smallest relative gap (d_next - d_min) / d_min over the queries with d_min > 0, d_next the smallest distance STRICTLY
    above d_min (coincident candidates tie exactly in every precision and are decided by index, not by rounding)."""
    p1, p2 = p1.double(), p2.double()
    B, N, D = p1.shape
    M = p2.shape[1]
    gap = float("inf")
    step = _rows_per_chunk(B, M, D, budget)
    for r in range(0, N, step):
        diff = p1[:, r:r + step, None, :] - p2[:, None, :, :]
        dd = (diff * diff).sum(-1).sqrt()
        lo = dd.min(dim=2, keepdim=True)[0]
        nxt = torch.where(dd > lo, dd, float("inf")).min(dim=2)[0]
        lo = lo[:, :, 0]
        live = (lo > 0) & torch.isfinite(nxt)
        if bool(live.any()):
            gap = min(gap, float(((nxt[live] - lo[live]) / lo[live]).min()))
    return gap


def distance_to(p1, p2, idx):
    """fp64 distance of every query to the candidate idx [B,N] names."""
    p1, p2 = p1.double(), p2.double()
    chosen = torch.gather(p2, 1, idx[:, :, None].expand(-1, -1, p2.shape[2]))
    return (p1 - chosen).pow(2).sum(-1).sqrt()


def value(d):
    return d.sum() / d.shape[0]


def gradients(p1, p2, idx, g):
    """The two gradients for the upstream scalar g, with the arg-min decisions given (idx [B,N]); also the number of queries
    that chose each candidate (count [B,M])."""
    p1, p2 = p1.double(), p2.double()
    B, N, D = p1.shape
    M = p2.shape[1]
    chosen = torch.gather(p2, 1, idx[:, :, None].expand(-1, -1, D))
    diff = p1 - chosen
    d = diff.pow(2).sum(-1, keepdim=True).sqrt()
    dp1 = torch.where(d > 0, (float(g) / B) * diff / torch.where(d > 0, d, torch.ones_like(d)), torch.zeros_like(diff))
    dp2 = torch.zeros(B, M, D, dtype=torch.float64, device=p1.device)
    dp2.scatter_add_(1, idx[:, :, None].expand(-1, -1, D), -dp1)
    count = torch.zeros(B, M, dtype=torch.float64, device=p1.device)
    count.scatter_add_(1, idx, torch.ones(B, N, dtype=torch.float64, device=p1.device))
    return dp1, dp2, count


def stock_chamfer(p1, p2):
    """What the HIP kernels replace: every pairwise difference as one broadcast tensor [B,N,M,D], its norm, the min over the
    candidates, the sum over queries and the mean over the batch -- stock torch in the inputs' dtype, differentiable."""
    diff = p1[:, :, None, :] - p2[:, None, :, :]
    return diff.norm(p=2, dim=3).min(dim=2)[0].sum() / p1.shape[0]


# Bounds of the issue this module was written for (derived from the number formats, not measured):
#   per point  |dist - d64| <= 2e-6 d64  (exact fp32 inputs, one rounding per difference, D squares, D - 1 adds, one square root:
#              about (D + 4) 2^-24 <= 8e-7 at D = 9, a factor of two on top);  dist == 0 exactly where d64 == 0
#   value      5e-6 relative (the per-point bound plus ordered blocked summation over <= 2^20 terms)
#   dp1        3e-6 |g| / B per component;  dp2[b,m]  4e-6 (|g| / B) max(1, count[b,m]);  zero rows exactly zero
#   choice     d64(p1[n], p2[idx[n]]) <= (1 + 4e-6) min_m d64  where the arg-min is not demanded exactly
DIST_REL, VALUE_REL, DP1_ABS, DP2_ABS, CHOICE_REL = 2e-6, 5e-6, 3e-6, 4e-6, 4e-6


def check_against(p1, p2, g, dist, idx, val, dp1, dp2, exact_idx=None, what=""):
    """Asserts every bound above for results (any float dtype, any device) of the inputs p1, p2 and the upstream scalar g.
    exact_idx: the arg-min that idx must equal everywhere; None: idx only has to be a (1 + 4e-6)-nearest candidate, and the
    gradients are evaluated at the decisions idx holds.  dist / idx / val / dp1 / dp2 may each be None (not checked).
    Returns the figures it compared, for printing."""
    B = p1.shape[0]
    d64, i64 = nearest(p1, p2)
    fig = {}
    if exact_idx is not None:
        wrong = int((idx != exact_idx.to(idx.device)).sum())
        assert wrong == 0, "%s: %d arg-min entries differ from the fp64 arg-min" % (what, wrong)
        assert bool((i64 == exact_idx.to(i64.device)).all()), "%s: the yardstick's own arg-min differs from the recorded one" % what
        chosen = d64
    else:
        assert bool(((idx >= 0) & (idx < p2.shape[1])).all()), "%s: idx out of range" % what
        chosen = distance_to(p1, p2, idx)
        slack = float((chosen / torch.where(d64 > 0, d64, torch.ones_like(d64)) - 1)[d64 > 0].max()) if bool((d64 > 0).any()) else 0.0
        fig["choice_rel"] = slack
        assert bool((chosen <= (1 + CHOICE_REL) * d64).all()), "%s: a chosen candidate is %.3g (relative) farther than the nearest" % (what, slack)
    if dist is not None:
        err = (dist.double() - chosen).abs()
        fig["dist_rel"] = float((err / torch.where(chosen > 0, chosen, torch.ones_like(chosen))).max())
        assert bool((err <= DIST_REL * chosen).all()), "%s: dist off by %.3g (relative)" % (what, fig["dist_rel"])
        assert bool((dist[chosen == 0] == 0).all()), "%s: dist != 0 at a coincident pair" % what
    if val is not None:
        want = float(value(d64))                                      # the true minimum, whatever idx chose
        fig["value_rel"] = abs(float(val) - want) / max(abs(want), 1e-300)
        assert abs(float(val) - want) <= VALUE_REL * abs(want), "%s: value %.9g vs %.9g" % (what, float(val), want)
    if dp1 is not None or dp2 is not None:
        r1, r2, count = gradients(p1, p2, idx, g)
        unit = abs(float(g)) / B
        if dp1 is not None:
            fig["dp1_abs/unit"] = float((dp1.double() - r1).abs().max()) / unit
            assert fig["dp1_abs/unit"] <= DP1_ABS, "%s: dp1 off by %.3g |g|/B" % (what, fig["dp1_abs/unit"])
            assert bool((dp1[(chosen == 0)] == 0).all()), "%s: dp1 row not exactly zero at distance 0" % what
        if dp2 is not None:
            rel = (dp2.double() - r2).abs().amax(dim=2) / (unit * count.clamp(min=1))
            fig["dp2_abs/(unit*max(1,c))"] = float(rel.max())
            assert float(rel.max()) <= DP2_ABS, "%s: dp2 off by %.3g (|g|/B) max(1,c)" % (what, float(rel.max()))
            live = torch.zeros_like(count).scatter_add_(1, idx, (chosen > 0).double())      # contributors at non-zero distance
            assert bool((dp2[live == 0] == 0).all()), "%s: dp2 row without a contribution is not exactly zero" % what
    return fig


# ---------------------------------------------------------------------------------------------------------------- launch plans
# csrc/chamfer.hip's make_plan in Python, held to the library by pn2_chamfer_nn_workspace_bytes (tests/test_chamfer_plans_cpu.py):
# a workgroup owns 256 * qpt queries of one cloud and one range of `chunk` candidates, which pass through LDS in tiles of
# tile_rows(D) rows; `splits` ranges are joined by a second kernel; `partials` fp64 sums are added by a third.
THREADS, MAX_SPLITS, MIN_CHUNK, MAX_D = 256, 64, 128, 16


def cdiv(a, b):
    return -(-a // b)


def tile_rows(D):
    """Candidates per LDS tile (CT): rows are pitched to DP = round4(D) floats and a tile is 16 KiB."""
    dp = (D + 3) & ~3
    return 1024 if dp <= 4 else 512 if dp <= 8 else 256


def plan(B, N, M, cus):
    """-> qpt, qtiles, splits, chunk, partials for a device of `cus` compute units."""
    target = 2 * cus
    max_splits = min(MAX_SPLITS, cdiv(M, MIN_CHUNK))
    qpt = 1 if B * cdiv(N, THREADS * 4) * max_splits < target else 4
    qtiles = cdiv(N, THREADS * qpt)
    wgs = B * qtiles
    want = max(1, min(max_splits, cdiv(target, wgs)))
    chunk = cdiv(cdiv(M, want), MIN_CHUNK) * MIN_CHUNK
    splits = cdiv(M, chunk)
    partials = wgs if splits == 1 else cdiv(B * N, THREADS)
    return qpt, qtiles, splits, chunk, partials


def workspace_bytes(B, N, M, cus):
    _, _, splits, _, partials = plan(B, N, M, cus)
    return ((8 * partials + 255) & ~255) + (8 * B * N * splits if splits > 1 else 0)


def tiles(M, chunk, ct):
    """[(first row, rows)] of every LDS tile of every candidate range, in the order the kernel visits them."""
    out = []
    for m0 in range(0, M, chunk):
        m1 = min(M, m0 + chunk)
        out += [(base, min(ct, m1 - base)) for base in range(m0, m1, ct)]
    return out


# ------------------------------------------------------------------------------------------------------------------ exact data
LATTICE = 8          # coordinates are k / 8, k = -16 .. 16


def lattice_clouds(seed, B, N, M, D):
    """CPU float32 p1 [B,N,D], p2 [B,M,D] whose coordinates are integer multiples of 1/8 in [-2, 2]: every difference, square and
    partial sum of d2 (<= 16 * 16 = 256, in steps of 1/64) is exact in fp32, so d2 is ONE number in every precision and order."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    p1 = torch.randint(-2 * LATTICE, 2 * LATTICE + 1, (B, N, D), generator=gen).float() / LATTICE
    p2 = torch.randint(-2 * LATTICE, 2 * LATTICE + 1, (B, M, D), generator=gen).float() / LATTICE
    return p1, p2


def exact_nearest(p1, p2, budget=1 << 28):
    """Lattice clouds (any device) -> (dist [B,N] float32, idx [B,N] int64): the arg-min on exact integers (coordinates times 8 as
    int64), the LOWEST index of the minimum; dist = the float32 square root of the exact d2 (numpy's is correctly rounded)."""
    a, b = torch.round(p1.double() * LATTICE).to(torch.int64), torch.round(p2.double() * LATTICE).to(torch.int64)
    assert bool((a.double() / LATTICE == p1.double()).all()) and bool((b.double() / LATTICE == p2.double()).all()), "not on the lattice"
    B, N, D = a.shape
    M = b.shape[1]
    d2 = torch.empty(B, N, dtype=torch.int64, device=a.device)
    idx = torch.empty(B, N, dtype=torch.int64, device=a.device)
    order = torch.arange(M, device=a.device)
    step = max(1, int(budget // (8 * B * M * 3)))
    for r in range(0, N, step):
        acc = torch.zeros(B, min(step, N - r), M, dtype=torch.int64, device=a.device)
        for k in range(D):
            t = a[:, r:r + step, None, k] - b[:, None, :, k]
            acc += t * t
        lo = acc.min(dim=2, keepdim=True)[0]
        idx[:, r:r + step] = torch.where(acc == lo, order, M).min(dim=2)[0]
        d2[:, r:r + step] = lo[:, :, 0]
    assert int(d2.max()) < 1 << 24                                       # the integer is exact as a float32
    dist = np.sqrt(d2.cpu().numpy().astype(np.float32) / np.float32(LATTICE * LATTICE))
    return torch.from_numpy(dist).to(p1.device), idx


def plant_twins(p1, p2, pairs, step=None):
    """In place, on CPU tensors.  For each (q, m_lo, m_hi) -- q a query counted over the flattened [B*N] rows, m_lo <= m_hi
    candidates of q's cloud -- sets p2[m_lo] = p2[m_hi] = p1[q] + e: an exact duplicate (the only way continuous data ties) that is
    the nearest candidate of q, so idx[q] must be m_lo.  e lies along one axis; its length is a quarter of q's nearest distance
    before the planting (relative gap 3 to whatever was there), or, with step given (lattice data), one lattice step towards 0:
    d2 = step^2, the smallest non-zero value there is.  Asserts on continuous data that the twins are q's nearest by a relative gap
    >= 1e-3 (nearest_gap) once every pair is planted, and that fp64 picks m_lo."""
    B, N, D = p1.shape
    used = set()
    for q, m_lo, m_hi in pairs:
        b, n = divmod(q, N)
        assert 0 <= m_lo <= m_hi < p2.shape[1] and not {(b, m_lo), (b, m_hi)} & used, (q, m_lo, m_hi)
        used |= {(b, m_lo), (b, m_hi)}
        axis = q % D
        e = torch.zeros(D)
        if step is None:
            d0, _ = nearest(p1[b:b + 1, n:n + 1], p2[b:b + 1])
            assert float(d0) > 0
            e[axis] = 0.25 * float(d0)
        else:
            e[axis] = -step if float(p1[b, n, axis]) > 0 else step
        p2[b, m_lo] = p2[b, m_hi] = p1[b, n] + e
        assert bool((p2[b, m_lo] != p1[b, n]).any())
    if step is None:
        for q, m_lo, m_hi in pairs:
            b, n = divmod(q, N)
            assert nearest_gap(p1[b:b + 1, n:n + 1], p2[b:b + 1]) >= 1e-3, (q, m_lo, m_hi)
            assert int(nearest(p1[b:b + 1, n:n + 1], p2[b:b + 1])[1]) == m_lo, (q, m_lo, m_hi)
    return p1, p2


# ------------------------------------------------------------------------------------------------------------------- the cases
# One list for tests/test_chamfer_abi_gpu.py (which launches them) and tests/test_chamfer_plans_cpu.py (which shows, for 256, 304
# and 64 compute units, that each reaches the branch it is named for and that its planted ties tell wrong tie rules apart).
def branch(B, N, M, D, cus):
    """The facts that name a launch plan's branch."""
    qpt, qtiles, splits, chunk, partials = plan(B, N, M, cus)
    tl = tiles(M, chunk, tile_rows(D))
    per_range = max(sum(1 for base, _ in tl if m0 <= base < m0 + chunk) for m0 in range(0, M, chunk))
    return dict(qpt=qpt, one_pass=splits == 1, tiles2=per_range >= 2, tiles=per_range, ragged=any(cnt % 4 for _, cnt in tl),
                qtiles2=qtiles >= 2, partials_gt_256=partials > THREADS, splits=splits, chunk=chunk, partials=partials,
                last_range=M - (splits - 1) * chunk, last_tile=tl[-1][1])


def cases(cus):
    """[(name, (B, N, M, D), facts the plan must show)] for a device of `cus` compute units.  The shapes are the smallest that
    reach each branch; B follows the device so that B * qtiles crosses 2 * cus on the intended side."""
    out = []
    one_pass_q4 = dict(qpt=4, one_pass=True, tiles=3, ragged=True, last_tile=3)
    for D in (3, 6, 11, 1, 2, 5, 7, 8, 13):
        out.append(("q4-onepass-3tiles-D%d" % D, (2 * cus, 5, 2 * tile_rows(D) + 3, D), one_pass_q4))
    # (at 64 compute units 2 * cus clouds would give exactly 256 partials: B is held above 128 so that the sum kernel's loop strides)
    out.append(("q4-onepass-2qtiles-strided-sum", (max(2 * cus, 160), 1025, 129, 3),
                dict(qpt=4, one_pass=True, qtiles2=True, partials_gt_256=True, tiles=1)))
    for D in (9, 16):
        out.append(("q1-onepass-2tiles-D%d" % D, (cus // 2, 1024, 300, D), dict(qpt=1, one_pass=True, tiles=2, ragged=False, last_tile=44)))
    joined_q1 = dict(qpt=1, one_pass=False, tiles=2, qtiles2=True, ragged=True)
    out.append(("q1-joined-2tiles-D3", (1, 300, 65541, 3), dict(joined_q1, last_range=1029, last_tile=5)))
    for D in (12, 1, 2, 5, 7, 8, 13):
        out.append(("q1-joined-2tiles-D%d" % D, (1, 300, 64 * tile_rows(D) + 6, D), joined_q1))
    out.append(("q4-joined-2tiles-D12", (cdiv(2 * cus, 128), 1025, 16390, 12), dict(qpt=4, one_pass=False, tiles=2, qtiles2=True, ragged=True)))
    out.append(("smallest-join", (1, 1, 129, 3), dict(qpt=1, one_pass=False, splits=2, last_range=1, tiles=1)))
    out.append(("control-one-tile", (3, 64, 64, 3), dict(qpt=1, one_pass=True, tiles=1, partials_gt_256=False)))
    return out


def seeded(seed, B, N, M, D):
    """Continuous CPU clouds, uniform in [-1, 1)."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return torch.rand(B, N, D, generator=gen) * 2 - 1, torch.rand(B, M, D, generator=gen) * 2 - 1


def case_clouds(kind, k, B, N, M, D, cus):
    """The CPU inputs of case number k: kind "lattice" (exact everywhere) or "twins" (continuous, exact duplicates planted), both
    with a pair on every seam of the plan -> p1, p2, [(seam, q, m_lo, m_hi)]."""
    pairs = seam_pairs(B, N, M, D, cus)
    if kind == "lattice":
        p1, p2 = lattice_clouds(100 + k, B, N, M, D)
        plant_twins(p1, p2, [p[1:] for p in pairs], step=1.0 / LATTICE)
    else:
        p1, p2 = seeded(200 + k, B, N, M, D)
        plant_twins(p1, p2, [p[1:] for p in pairs])
    return p1, p2, pairs


def seam_pairs(B, N, M, D, cus):
    """The (q, m_lo, m_hi) that plant_twins gets for a case: one pair per seam the case's plan has, each on a query of its own
    (spread over the clouds when N is small) -> [(seam, q, m_lo, m_hi)].
      a  two rows of one 4-group              b  the last row of the unrolled body and the first of the remainder
      r  one candidate alone in the remainder (the LAST row of a ragged tile)
      c  rows CT-1 and CT of one range        d  rows chunk-1 and chunk        e  the first and the last range"""
    _, _, splits, chunk, _ = plan(B, N, M, cus)
    ct = tile_rows(D)
    tl = tiles(M, chunk, ct)
    want = []                                                # (in the order they are kept when there are fewer queries than seams)
    if splits > 1:
        m0 = chunk * (2 if splits > 3 else 1)
        want.append(("d", m0 - 1, m0))
    if min(chunk, M) > ct:
        m0 = chunk if splits > 2 else 0                      # (a middle range where there is one)
        want.append(("c", m0 + ct - 1, m0 + ct))
    ragged = [(base, cnt) for base, cnt in tl if cnt % 4]
    if ragged:
        base, cnt = ragged[-1]
        if cnt > 4:
            want.append(("b", base + (cnt & ~3) - 1, base + (cnt & ~3)))
        if cnt % 4 > 1:
            want.append(("r", base + cnt - 1, base + cnt - 1))
    if splits > 2:
        want.append(("e", 1, (splits - 1) * chunk))
    if M >= 8:
        want.append(("a", 4, 5))
    total = B * N
    want = want[:total]
    rows = [m for _, lo, hi in want for m in (lo, hi)]
    assert len(set(rows)) == len(rows) - sum(1 for _, lo, hi in want if lo == hi), want
    return [(seam, i * (total // len(want)), lo, hi) for i, (seam, lo, hi) in enumerate(want)]
