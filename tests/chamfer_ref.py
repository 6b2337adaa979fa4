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
