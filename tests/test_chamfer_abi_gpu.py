"""GPU: pn2_chamfer_nn and pn2_chamfer_bwd at the C ABI (ctypes, raw pointers), on every launch plan csrc/chamfer.hip can take.

The shapes are chamfer_ref.cases(compute units of this device): each is asserted against the restated plan before its launch and
prints the plan it ran (tests/test_chamfer_plans_cpu.py holds the restatement to the library and the list to its branches).
Every output and the workspace sit between 64 guard words that must come back unchanged; the workspace is 256-byte aligned and
filled with a NaN bit pattern (it need not be cleared); every forward runs twice, with `sum` and with sum = NULL, which must give
the same dist and idx bits and leave the sum word alone.

  lattice data (coordinates k / 8: d2 is exact in every precision and order, ties are plentiful, a pair planted on every seam of
      the plan): idx EQUALS the integer arg-min everywhere, dist its correctly rounded square root bit for bit, and sum equals
      f32(S) / f32(B) in fp32 for S = math.fsum(dist), or that with f32(S) moved one ulp either way (the kernel adds the same
      terms in fp64 in another order and rounds once); which of the three matched is printed.
  continuous data with exact duplicates planted across every seam (two rows of a 4-group; unrolled body / remainder; the last row
      of a ragged tile; rows CT-1 / CT; rows chunk-1 / chunk; first / last range) and one query that coincides with a candidate:
      idx at a planted query is the LOWER twin, everything else meets chamfer_ref.check_against as in test_chamfer_gpu.py.
  backward with the kernel's own dist and idx: chamfer_ref's bounds DP1_ABS / DP2_ABS, dp1 = NULL and dp2 = NULL each alone, both
      NULL, idx entries of -1 and M (zero dp1 rows, nothing added to dp2), all N queries on one candidate.
  refusals launch nothing; non-finite coordinates do what include/pn2.h says.

Measured on an MI355X (256 compute units), after the checks were written.  The first run failed its first lattice case on dist:
__fsqrt_rn was the native one-ulp root; the kernels now call sqrtf.  Since then all 23 lattice cases match the un-moved
f32(S) / f32(B), the worst dp1 error is 0.06 of DP1_ABS and the worst dp2 error 0.06 of DP2_ABS."""
import math

import numpy as np
import pytest
import torch

import chamfer_ref as C

from pointnet12_amd import _lib

pytestmark = pytest.mark.gpu

EINVAL = -1
GUARD = 64
F_SENT, I_SENT = -777.0, -777
WS_FILL, WS_GUARD = 0x7FC00000, 0x7FC0ABCD          # both are NaNs as floats, and as the halves of a double
NAMES = [name for name, _, _ in C.cases(256)]
G = -0.625


class Frame:
    """n elements between GUARD guard words on either side; the first element is 256-byte aligned."""

    def __init__(self, dev, n, dtype, guard, fill=None):
        self.n, self.guard = n, guard
        self.hold = torch.full((n + 2 * GUARD,), guard, dtype=dtype, device=dev)
        self.view = self.hold[GUARD:GUARD + n]
        if fill is not None:
            self.view.fill_(fill)
        self.ptr = self.view.data_ptr()
        assert self.ptr % 256 == 0

    def intact(self, what):
        front, back = self.hold[:GUARD].cpu(), self.hold[GUARD + self.n:].cpu()
        assert bool((front == self.guard).all()) and bool((back == self.guard).all()), "a guard word of %s was written" % what

    def untouched(self, what, value):
        self.intact(what)
        assert bool((self.view == value).all()), "%s was written" % what


def bits(t):
    return t.contiguous().view(torch.int32)


def cus_of(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def forward(dev, a, b, want_sum=True):
    """-> dist [B,N], idx [B,N], sum (0-dim, or None), after the guard checks."""
    lib = _lib.load()
    B, N, D = a.shape
    M = b.shape[1]
    nbytes = lib.pn2_chamfer_nn_workspace_bytes(B, N, M, D)
    assert nbytes == C.workspace_bytes(B, N, M, cus_of(dev)) and nbytes % 4 == 0
    ws = Frame(dev, nbytes // 4, torch.int32, WS_GUARD, WS_FILL)
    dist, idx = Frame(dev, B * N, torch.float32, F_SENT), Frame(dev, B * N, torch.int64, I_SENT)
    total = Frame(dev, 1, torch.float32, F_SENT)
    rc = lib.pn2_chamfer_nn(a.data_ptr(), b.data_ptr(), B, N, M, D, dist.ptr, idx.ptr, total.ptr if want_sum else None, ws.ptr,
                            _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0
    for f, what in ((ws, "workspace"), (dist, "dist"), (idx, "idx"), (total, "sum")):
        f.intact(what)
    if not want_sum:
        total.untouched("sum (NULL was passed)", F_SENT)
    return dist.view.view(B, N).clone(), idx.view.view(B, N).clone(), total.view[0].clone() if want_sum else None


def backward(dev, a, b, dist, idx, g, want1=True, want2=True):
    """-> rc, dp1 [B,N,D], dp2 [B,M,D] (dp2 starts from zeros; an output that was not asked for must keep its fill)."""
    lib = _lib.load()
    B, N, D = a.shape
    M = b.shape[1]
    dp1, dp2 = Frame(dev, B * N * D, torch.float32, F_SENT, 123.0), Frame(dev, B * M * D, torch.float32, F_SENT, 0.0)
    gd = torch.tensor([g], device=dev, dtype=torch.float32)
    assert dist.is_contiguous() and idx.is_contiguous() and idx.dtype == torch.int64
    rc = lib.pn2_chamfer_bwd(a.data_ptr(), b.data_ptr(), dist.data_ptr(), idx.data_ptr(), gd.data_ptr(), B, N, M, D,
                             dp1.ptr if want1 else None, dp2.ptr if want2 else None, _lib.stream())
    torch.cuda.synchronize()
    dp1.intact("dp1")
    dp2.intact("dp2")
    if not want1:
        dp1.untouched("dp1 (NULL was passed)", 123.0)
    if not want2:
        dp2.untouched("dp2 (NULL was passed)", 0.0)
    return rc, dp1.view.view(B, N, D).clone(), dp2.view.view(B, M, D).clone()


def both_forwards(dev, a, b):
    dist, idx, total = forward(dev, a, b, True)
    dist2, idx2, _ = forward(dev, a, b, False)
    assert torch.equal(bits(dist), bits(dist2)) and torch.equal(idx, idx2), "sum = NULL changed dist or idx"
    return dist, idx, total


def backward_variants(dev, a, b, dist, idx, g, what, exact_idx=None):
    """Both outputs, each alone, neither; -> dp1, dp2 and the figures of check_against."""
    rc, dp1, dp2 = backward(dev, a, b, dist, idx, g)
    assert rc == 0
    fig = C.check_against(a, b, g, None, idx, None, dp1, dp2, exact_idx=exact_idx, what=what)
    rc, only1, _ = backward(dev, a, b, dist, idx, g, want2=False)
    assert rc == 0 and torch.equal(bits(only1), bits(dp1)), "%s: dp1 differs when dp2 = NULL" % what
    rc, _, only2 = backward(dev, a, b, dist, idx, g, want1=False)
    assert rc == 0
    C.check_against(a, b, g, None, idx, None, None, only2, exact_idx=exact_idx, what=what + ", dp1 = NULL")
    rc, _, _ = backward(dev, a, b, dist, idx, g, want1=False, want2=False)
    assert rc == 0
    return dp1, dp2, fig


def out_of_range_idx(dev, a, b, dist, idx, g, dp1, what):
    """Entries of idx set to -1 and to M: their dp1 rows are exactly zero, they add nothing to dp2, everything else is as before."""
    B, N, D = a.shape
    M = b.shape[1]
    r1, r2, count = C.gradients(a, b, idx, g)
    chosen_count = torch.gather(count, 1, idx)
    alone = ((chosen_count == 1) & (dist > 0)).view(-1).nonzero().view(-1).tolist()        # their candidate's dp2 row must end as zeros
    qs = (alone + [q for q in range(B * N) if q not in alone[:2]][:2])[:2]
    plants = [list(zip(qs, (-1, M)))] if len(qs) == 2 else [[(qs[0], -1)], [(qs[0], M)]]
    unit = abs(g) / B
    for plant in plants:
        bad, want2, cnt = idx.clone(), r2.clone(), count.clone()
        for q, value in plant:
            bb, n = divmod(q, N)
            want2[bb, idx[bb, n]] += r1[bb, n]
            cnt[bb, idx[bb, n]] -= 1
            bad[bb, n] = value
        rc, got1, got2 = backward(dev, a, b, dist, bad, g)
        assert rc == 0
        keep = torch.ones(B * N, dtype=torch.bool, device=a.device)
        keep[[q for q, _ in plant]] = False
        assert torch.equal(bits(got1).view(B * N, D)[keep], bits(dp1).view(B * N, D)[keep]), "%s: another query's dp1 moved" % what
        assert bool((bits(got1).view(B * N, D)[~keep] == 0).all()), "%s: dp1 row of an out-of-range idx is not +0" % what
        rel = (got2.double() - want2).abs().amax(dim=2) / (unit * cnt.clamp(min=1))
        assert float(rel.max()) <= C.DP2_ABS, "%s: dp2 off by %.3g with out-of-range idx" % (what, float(rel.max()))
        assert bool((got2[cnt == 0] == 0).all()), "%s: an out-of-range idx added to dp2" % what


def announce(dev, kind, name, shape):
    B, N, M, D = shape
    cus = cus_of(dev)
    got = C.branch(B, N, M, D, cus)
    print("chamfer %-8s %-32s B %d N %d M %d D %d  CUs %d  qpt %d qtiles %d splits %d chunk %d CT %d tiles/range %d last tile %d "
          "partials %d" % (kind, name, B, N, M, D, cus, got["qpt"], C.plan(B, N, M, cus)[1], got["splits"], got["chunk"],
                           C.tile_rows(D), got["tiles"], got["last_tile"], got["partials"]))
    return cus


def case(dev, k):
    """Case k for this device, its facts asserted against the restated plan BEFORE anything is launched."""
    cus = cus_of(dev)
    name, shape, facts = C.cases(cus)[k]
    assert name == NAMES[k]
    got = C.branch(*shape, cus)
    for key, want in facts.items():
        assert got[key] == want, "the planner no longer takes case %s where it was aimed: %s is %s" % (name, key, got[key])
    return name, shape


# ------------------------------------------------------------------------------------------------------------ 1. lattice data
@pytest.mark.parametrize("k", range(len(NAMES)), ids=NAMES)
def test_lattice_data_is_exact(dev, k):
    name, (B, N, M, D) = case(dev, k)
    cus = announce(dev, "lattice", name, (B, N, M, D))
    p1, p2, pairs = C.case_clouds("lattice", k, B, N, M, D, cus)
    a, b = p1.to(dev), p2.to(dev)
    dist, idx, total = both_forwards(dev, a, b)
    want_dist, want_idx = C.exact_nearest(a, b)
    wrong = idx != want_idx
    assert not bool(wrong.any()), "%s: %d of %d arg-mins differ from the integer arg-min, first at %s" % (
        name, int(wrong.sum()), wrong.numel(), wrong.nonzero()[0].tolist())
    assert torch.equal(bits(dist), bits(want_dist)), "%s: dist is not the correctly rounded root of the exact d2" % name
    # sum: f32(S) / f32(B) in fp32, f32(S) moved by at most one ulp
    S = math.fsum(dist.double().cpu().view(-1).tolist())
    s0 = np.float32(S)
    cands = (("f32(S)", s0), ("f32(S) - 1 ulp", np.nextafter(s0, np.float32(-np.inf))), ("f32(S) + 1 ulp", np.nextafter(s0, np.float32(np.inf))))
    got = np.float32(total.item())
    matched = [label for label, c in cands if np.float32(c / np.float32(B)).view(np.uint32) == got.view(np.uint32)]
    print("    sum %.9g: matched %s; ties at the planted seams: %s" % (
        float(got), matched[0] if matched else "NONE (S = %.17g)" % S,
        ", ".join("%s->%d" % (seam, int(idx.view(-1)[q])) for seam, q, _, _ in pairs)))
    assert matched, "%s: sum %.9g is none of f32(S) / B with f32(S) moved by -1, 0, +1 ulp (S = %.17g)" % (name, float(got), S)
    _, _, fig = backward_variants(dev, a, b, dist, idx, G, name, exact_idx=want_idx)
    print("    backward", fig)


# --------------------------------------------------------------------------------------------- 2. continuous data, planted twins
@pytest.mark.parametrize("k", range(len(NAMES)), ids=NAMES)
def test_planted_twins_and_fp64_bounds(dev, k):
    name, (B, N, M, D) = case(dev, k)
    cus = announce(dev, "twins", name, (B, N, M, D))
    p1, p2, pairs = C.case_clouds("twins", k, B, N, M, D, cus)
    qz = B * N - 1                                                  # one query on top of a candidate
    zero = qz not in [q for _, q, _, _ in pairs]
    if zero:
        bz, nz, mz = qz // N, qz % N, (2 if M > 8 else 0)
        p1[bz, nz] = p2[bz, mz]
    a, b = p1.to(dev), p2.to(dev)
    dist, idx, total = both_forwards(dev, a, b)
    for seam, q, lo, hi in pairs:
        assert int(idx.view(-1)[q]) == lo, "%s: seam %s: twins %d / %d, the kernel chose %d" % (name, seam, lo, hi, int(idx.view(-1)[q]))
    dp1, dp2, _ = backward_variants(dev, a, b, dist, idx, G, name)
    fig = C.check_against(a, b, G, dist, idx, total, dp1, dp2, what=name)
    print("    seams %s  %s" % ("".join(s for s, _, _, _ in pairs), fig))
    if zero:
        assert int(idx[bz, nz]) == mz and float(dist[bz, nz]) == 0.0 and bool((bits(dp1[bz, nz]) == 0).all())
        _, _, count = C.gradients(a, b, idx, G)
        if int(count[bz, mz]) == 1:                                 # nobody else chose it: nothing may have been added
            assert bool((bits(dp2[bz, mz]) == 0).all())
    out_of_range_idx(dev, a, b, dist, idx, G, dp1, name)


# ------------------------------------------------------------------------------------------------- 3. every query, one candidate
def test_every_query_chooses_one_candidate(dev):
    """300 queries in [-2, 0]^3, candidates in [1, 2]^3 except number 77 at (1/8, 1/8, 1/8): dp2[b, 77] gathers 300 atomics, every
    other row stays zero; the bound scales with the count (chamfer_ref.DP2_ABS)."""
    B, N, M, D = 2, 300, 140, 3
    announce(dev, "lattice", "one-candidate", (B, N, M, D))
    p1, p2 = C.lattice_clouds(5, B, N, M, D)
    p1, p2 = -p1.abs(), 1 + p2.abs() / 2
    p2 = (p2 * 8).round() / 8
    p2[:, 77] = 0.125
    a, b = p1.to(dev), p2.to(dev)
    dist, idx, total = both_forwards(dev, a, b)
    want_dist, want_idx = C.exact_nearest(a, b)
    assert bool((want_idx == 77).all()) and torch.equal(idx, want_idx) and torch.equal(bits(dist), bits(want_dist))
    dp1, dp2, fig = backward_variants(dev, a, b, dist, idx, G, "one candidate", exact_idx=want_idx)
    print("    backward", fig)
    rest = torch.ones(M, dtype=torch.bool, device=dev)
    rest[77] = False
    assert bool((bits(dp2[:, rest]) == 0).all()) and bool((dp2[:, 77] != 0).any())
    out_of_range_idx(dev, a, b, dist, idx, G, dp1, "one candidate")


# ------------------------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_launch_nothing(dev):
    lib = _lib.load()
    B, N, M, D = 2, 70, 140, 3
    p1, p2 = C.seeded(11, B, N, M, D)
    a, b = p1.to(dev), p2.to(dev)
    dist0, idx0, _ = forward(dev, a, b)
    ws = Frame(dev, lib.pn2_chamfer_nn_workspace_bytes(B, N, M, D) // 4, torch.int32, WS_GUARD, WS_FILL)
    dist, idx, total = Frame(dev, B * N, torch.float32, F_SENT), Frame(dev, B * N, torch.int64, I_SENT), Frame(dev, 1, torch.float32, F_SENT)
    dp1, dp2 = Frame(dev, B * N * D, torch.float32, F_SENT), Frame(dev, B * M * D, torch.float32, F_SENT)
    gd = torch.tensor([G], device=dev)
    st = _lib.stream()
    ok = dict(p1=a.data_ptr(), p2=b.data_ptr(), B=B, N=N, M=M, D=D, dist=dist.ptr, idx=idx.ptr, sum=total.ptr, ws=ws.ptr)

    def nn(**kw):
        v = dict(ok, **kw)
        return lib.pn2_chamfer_nn(v["p1"], v["p2"], v["B"], v["N"], v["M"], v["D"], v["dist"], v["idx"], v["sum"], v["ws"], st)

    for kw in (dict(p1=None), dict(p2=None), dict(dist=None), dict(idx=None), dict(ws=None), dict(B=0), dict(B=65536), dict(B=-1),
               dict(N=0), dict(M=0), dict(D=0), dict(N=-3), dict(M=-3), dict(D=-3)):
        assert nn(**kw) == EINVAL, kw
    assert nn(D=17) == _lib.PN2_EUNSUPPORTED
    okb = dict(p1=a.data_ptr(), p2=b.data_ptr(), dist=dist0.data_ptr(), idx=idx0.data_ptr(), g=gd.data_ptr(), B=B, N=N, M=M, D=D,
               dp1=dp1.ptr, dp2=dp2.ptr)

    def bwd(**kw):
        v = dict(okb, **kw)
        return lib.pn2_chamfer_bwd(v["p1"], v["p2"], v["dist"], v["idx"], v["g"], v["B"], v["N"], v["M"], v["D"], v["dp1"], v["dp2"], st)

    for kw in (dict(p1=None), dict(p2=None), dict(dist=None), dict(idx=None), dict(g=None), dict(B=0), dict(N=0), dict(M=0), dict(D=0),
               dict(B=-1), dict(D=-3)):
        assert bwd(**kw) == EINVAL, kw
    assert bwd(D=17) == _lib.PN2_EUNSUPPORTED
    assert bwd(dp1=None, dp2=None) == 0
    torch.cuda.synchronize()
    ws.untouched("workspace", WS_FILL)
    for f, what, value in ((dist, "dist", F_SENT), (idx, "idx", I_SENT), (total, "sum", F_SENT), (dp1, "dp1", F_SENT), (dp2, "dp2", F_SENT)):
        f.untouched(what, value)
    assert torch.equal(a.cpu(), p1) and torch.equal(b.cpu(), p2)


# --------------------------------------------------------------------------------------------------------- 5. non-finite inputs
def test_non_finite_coordinates(dev):
    """What include/pn2.h states: a d2 that is NaN or +inf never passes `d2 < best`, so a candidate with a NaN or infinite
    coordinate is never chosen and a query with one gets idx 0 and dist +inf (sum becomes +inf); such a row changes no other
    query's dist, idx or dp1 bits and, in dp2, only candidate 0 of its own cloud."""
    B, N, M, D = 2, 70, 140, 3
    announce(dev, "nonfinite", "non-finite", (B, N, M, D))
    nan, inf = float("nan"), float("inf")
    p1, p2 = C.seeded(12, B, N, M, D)
    bad_c = ((0, 5, 1, nan), (1, 9, 0, inf), (1, 139, 2, -inf), (0, 128, 0, nan))        # (cloud, candidate, component, value)
    bad_q = ((0, 3, 2, nan), (1, 8, 1, inf), (1, 69, 0, -inf))
    for bb, m, c, _ in bad_c:
        p2[bb, m] = 100.0                                           # baseline: far away, never the nearest
    for bb, n, c, _ in bad_q:
        p1[bb, n] = p2[bb, 0]                                       # baseline: on top of candidate 0, adds nothing anywhere
    a, b = p1.to(dev), p2.to(dev)
    dist0, idx0, total0 = both_forwards(dev, a, b)
    dp1_0, dp2_0, _ = backward_variants(dev, a, b, dist0, idx0, G, "non-finite baseline")
    assert not bool(sum((idx0[bb] == m).any() for bb, m, _, _ in bad_c))
    r1, r2, count = C.gradients(a, b, idx0, G)

    # candidates only: every result keeps its bits (dp2 up to the order of its atomics)
    q2 = p2.clone()
    for bb, m, c, v in bad_c:
        q2[bb, m, c] = v
    bq = q2.to(dev)
    dist, idx, total = both_forwards(dev, a, bq)
    assert torch.equal(bits(dist), bits(dist0)) and torch.equal(idx, idx0) and torch.equal(bits(total), bits(total0))
    rc, dp1, dp2 = backward(dev, a, bq, dist, idx, G)
    assert rc == 0 and torch.equal(bits(dp1), bits(dp1_0))
    unit = abs(G) / B
    single = count <= 1                                             # one atomic onto +0: the same bits
    assert torch.equal(bits(dp2)[single], bits(dp2_0)[single])
    assert float(((dp2.double() - r2).abs().amax(dim=2) / (unit * count.clamp(min=1))).max()) <= C.DP2_ABS

    # queries too
    q1 = p1.clone()
    for bb, n, c, v in bad_q:
        q1[bb, n, c] = v
    aq = q1.to(dev)
    dist, idx, total = both_forwards(dev, aq, bq)
    others = torch.ones(B, N, dtype=torch.bool, device=dev)
    for bb, n, _, _ in bad_q:
        others[bb, n] = False
        assert int(idx[bb, n]) == 0 and float(dist[bb, n]) == inf, (bb, n, int(idx[bb, n]), float(dist[bb, n]))
    assert torch.equal(bits(dist)[others], bits(dist0)[others]) and torch.equal(idx[others], idx0[others])
    assert float(total) == inf
    rc, dp1, dp2 = backward(dev, aq, bq, dist, idx, G)
    assert rc == 0 and torch.equal(bits(dp1)[others], bits(dp1_0)[others])
    rows = torch.ones(B, M, dtype=torch.bool, device=dev)
    rows[:, 0] = False                                              # candidate 0 of the cloud is where a non-finite query lands
    assert torch.equal(bits(dp2)[single & rows], bits(dp2_0)[single & rows])
    assert float(((dp2.double() - r2).abs().amax(dim=2) / (unit * count.clamp(min=1)))[rows].max()) <= C.DP2_ABS
    print("    observed: idx 0, dist +inf, sum +inf for the three non-finite queries; their dp1 rows %s; dp2[:, 0] %s" % (
        dp1[~others].tolist(), dp2[:, 0].tolist()))
