"""CPU: the launch plans of the Chamfer search (csrc/chamfer.hip: make_plan) as tests/chamfer_ref.py restates them, and the case list of
tests/test_chamfer_abi_gpu.py held to what it is for.

  1. chamfer_ref.workspace_bytes equals pn2_chamfer_nn_workspace_bytes (host code; the library assumes 256 compute units where it
     finds no device) on every shape the GPU files launch and on 400 drawn ones: the restated plan is the library's.
  2. For 256, 304 and 64 compute units every case of chamfer_ref.cases shows the branch it is named for, and every branch the
     issue lists occurs; at 256 compute units none of the older sweep's shapes takes the one-pass kernel past one 128-row tile.
  3. The planted ties discriminate: three wrong tie rules -- the HIGHEST index on equal d2; ranges joined with `<=` (the later
     range wins a tie); a tile search that drops the last cnt % 4 candidates -- each change idx exactly at the planted queries
     whose seam they break, on the continuous cases, and on at least one query of the lattice cases."""
import numpy as np
import pytest
import torch

import chamfer_ref as C
from test_chamfer_gpu import SWEEP

from pointnet12_amd import _lib

CUS = (256, 304, 64)


def library_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def test_restated_plan_gives_the_library_workspace_size():
    lib = _lib.load()
    cus = library_cus()
    shapes = [s[:3] for _, s, _ in C.cases(cus)] + list(SWEEP) + [(2, 300, 257), (1, 1111, 77), (2, 70, 140), (2, 300, 140)]
    rng = np.random.RandomState(7)
    for _ in range(400):
        top = (1024, 70000, 70000) if rng.rand() < 0.5 else (64, 3000, 3000)
        shapes.append(tuple(int(rng.randint(1, t + 1)) for t in top))
    for B, N, M in shapes:
        got = lib.pn2_chamfer_nn_workspace_bytes(B, N, M, 3)
        assert got == C.workspace_bytes(B, N, M, cus), ((B, N, M), C.plan(B, N, M, cus))
        assert got == lib.pn2_chamfer_nn_workspace_bytes(B, N, M, 16)                  # the plan does not depend on D
    assert [C.tile_rows(D) for D in range(1, 17)] == [1024] * 4 + [512] * 4 + [256] * 8


@pytest.mark.parametrize("cus", CUS)
def test_every_case_reaches_the_branch_it_names(cus):
    seen = set()
    for name, (B, N, M, D), facts in C.cases(cus):
        got = C.branch(B, N, M, D, cus)
        print(cus, name, (B, N, M, D), got)
        for key, want in facts.items():
            assert got[key] == want, (cus, name, key, got)
        assert B <= 65535 and B * N * M <= 100e6, name                                 # pair evaluations on the device
        seen.add((got["qpt"], got["one_pass"], got["tiles2"]))
        if got["ragged"] and got["tiles2"]:
            seen.add(("ragged last tile after a full one", got["one_pass"]))
        if got["qtiles2"]:
            seen.add(("two query tiles", got["qpt"], got["one_pass"]))
        if got["partials_gt_256"]:
            seen.add("strided sum")
        seen.add(("CT", C.tile_rows(D), got["one_pass"], got["tiles2"]))
        seen.add(("DP", (D + 3) & ~3, got["tiles2"]))
    for combo in [(4, True, True), (4, True, False), (1, True, True), (1, True, False), (1, False, True), (4, False, True),
                  (1, False, False), ("ragged last tile after a full one", True), ("ragged last tile after a full one", False),
                  ("two query tiles", 4, True), ("two query tiles", 1, True), ("two query tiles", 1, False), ("two query tiles", 4, False),
                  "strided sum"]:
        assert combo in seen, (cus, combo)
    for ct in (1024, 512, 256):                                    # both sides of each CT step, one pass and joined, past one tile
        assert ("CT", ct, True, True) in seen and ("CT", ct, False, True) in seen, ct
    for dp in (4, 8, 12, 16):
        assert ("DP", dp, True) in seen, dp


def test_the_older_sweep_never_ran_the_one_pass_kernel_past_one_tile():
    for B, N, M in SWEEP:
        _, _, splits, _, _ = C.plan(B, N, M, 256)
        assert not (splits == 1 and M > 128), (B, N, M)
    for B, N, M in ((2, 300, 257), (1, 1111, 77)):                  # test_every_point_dimension: one tile per range at every D
        assert C.plan(B, N, M, 256)[3] == 128


def rules(q, c, chunk, ct):
    """q [Q,D], c [M,D] of one cloud -> {rule: idx [Q]} from ONE fp64 d2 matrix (exact on the lattice; planted twins hold the same
    coordinates and so the same d2)."""
    q, c = q.double(), c.double()
    M = c.shape[0]
    d2 = torch.zeros(q.shape[0], M, dtype=torch.float64)
    for k in range(q.shape[1]):
        t = q[:, None, k] - c[None, :, k]
        d2 += t * t
    order = torch.arange(M)

    def lowest(x, live):
        hit = (x == torch.where(live, x, float("inf")).min(dim=1, keepdim=True)[0]) & live
        return hit, torch.where(hit, order, M).min(dim=1)[0]

    everything = torch.ones(M, dtype=torch.bool)
    hit, right = lowest(d2, everything)
    out = {"right": right, "highest": torch.where(hit, order, -1).max(dim=1)[0]}
    rng = order // chunk
    last = torch.where(hit, rng, -1).max(dim=1, keepdim=True)[0]
    out["le_join"] = torch.where(hit & (rng == last), order, M).min(dim=1)[0]
    keep = everything.clone()
    for base, cnt in C.tiles(M, chunk, ct):
        keep[base + (cnt & ~3):base + cnt] = False
    out["drop_tail"] = lowest(d2, keep)[1]
    return out


WRONG = ("highest", "le_join", "drop_tail")


@pytest.mark.parametrize("cus", CUS)
def test_planted_twins_tell_the_wrong_rules_apart(cus):
    """Continuous data: only the planted queries can tie, and each wrong rule must move exactly those whose seam it breaks."""
    moved = dict.fromkeys(WRONG, 0)
    seams = set()
    for k, (name, (B, N, M, D), _) in enumerate(C.cases(cus)):
        p1, p2, pairs = C.case_clouds("twins", k, B, N, M, D, cus)
        chunk, ct = C.plan(B, N, M, cus)[3], C.tile_rows(D)
        dropped = {m for base, cnt in C.tiles(M, chunk, ct) for m in range(base + (cnt & ~3), base + cnt)}
        for seam, qq, lo, hi in pairs:
            b, n = divmod(qq, N)
            got = {r: int(v) for r, v in rules(p1[b, n:n + 1], p2[b], chunk, ct).items()}
            assert got["right"] == lo, (name, seam)
            assert got["highest"] == hi, (name, seam)
            assert (got["le_join"] != lo) == (lo // chunk != hi // chunk), (name, seam, got)
            assert (got["drop_tail"] != lo) == (lo in dropped), (name, seam, got)
            if seam in "de":
                assert got["le_join"] == hi
            if seam == "b":
                assert hi in dropped and lo not in dropped and lo % 4 == 3
            if seam == "c":
                assert (lo % chunk) == ct - 1 and hi == lo + 1 and lo // chunk == hi // chunk
            if seam == "a":
                assert lo // 4 == hi // 4
            for r in WRONG:
                moved[r] += got[r] != lo
            seams.add(seam)
    print(cus, moved, sorted(seams))
    assert seams == set("abcder") and all(moved.values()), (moved, seams)


def test_lattice_cases_tell_the_wrong_rules_apart():
    """Exact data ties everywhere at low D: on the planted queries and the first 64 queries of cloud 0 of every case, each wrong
    rule moves idx somewhere, and the rule under test agrees with exact_nearest's integers."""
    cus = 256
    moved = dict.fromkeys(WRONG, 0)
    for k, (name, (B, N, M, D), _) in enumerate(C.cases(cus)):
        p1, p2, pairs = C.case_clouds("lattice", k, B, N, M, D, cus)
        chunk, ct = C.plan(B, N, M, cus)[3], C.tile_rows(D)
        rows = [(0, n) for n in range(min(N, 64))] + [divmod(qq, N) for _, qq, _, _ in pairs]
        here = dict.fromkeys(WRONG, 0)
        for b in sorted({b for b, _ in rows}):
            ns = torch.tensor([n for bb, n in rows if bb == b])
            got = rules(p1[b, ns], p2[b], chunk, ct)
            dist, idx = C.exact_nearest(p1[b:b + 1, ns], p2[b:b + 1])
            assert torch.equal(idx[0], got["right"]), name
            want = C.distance_to(p1[b:b + 1, ns], p2[b:b + 1], idx)                      # fp64 of exact squares: exact up to one sqrt
            assert bool((dist.double() - want).abs().max() <= 2.0 ** -24 * want.max()), name
            for r in WRONG:
                here[r] += int((got[r] != got["right"]).sum())
        print(name, (B, N, M, D), here)
        for r in WRONG:
            moved[r] += here[r]
    assert all(moved.values()), moved
