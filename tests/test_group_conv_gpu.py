"""GPU: pn2_group_conv_fwd (csrc/grouped.hip: gather + centre + concat + first conv + BatchNorm sums in one persistent,
software-pipelined launch) called through the C ABI and held to the fp64 statement of tests/fused_ref.py.

Assertions of every run: X bit-equal to the separately rounded float32 statement (pad columns zero); every element of Y
within the derived per-element bound E_1 = |W| E_0 + 1.05 (K + 2) u (|W| |x| + |b|), K = 3 + D <= 12; sum y and sum y^2
(summed over the replicas) within 1e-5 of sum |y| and sum y^2; X and Y sit in sentinel-filled buffers: rows behind P and
the columns [C_out, ldy) of Y still hold the sentinel, every element inside has been written; with stats == NULL Y has the
same bits.  Operands are drawn directly (no query, no FPS); every cloud's index holds 0, N - 1 and duplicates, B >= 2.

Coverage by construction.  C = the device's compute-unit count, the number the launcher caps its grid with
(min(cdiv(slabs, 4), 2 C) workgroups of four waves, one slab of 64 rows per wave and trip), so a wave w of 8 C makes
ceil((slabs - w) / (8 C)) trips; the first trip waits for everything (vmcnt(0)), every later one runs on the hand-counted
waits vmcnt(20/19) (C_out 64) or (12/11) (C_out 32):

    test_slab_counts
        slabs 1, 3, 5        a last (only) workgroup with waves that own no slab at all (3, 1, 3 of them); 4: none idle
        slabs 8 C - 1, 8 C   the capped grid, exactly one trip per wave (8 C - 1: the last wave owns nothing)
        slabs 8 C + 1, + 5   the first 1 / 5 waves take a second trip on the counted waits, all others do not
        slabs m6 = the first multiple of 6 above 8 C: two trips with K = 64, 3 and 96 whatever C is
        slabs 16 C + 1       three trips for wave 0, two for the rest
      each with every K of 16, 32, 64, 3, 96 for which B * S * K = 64 * slabs has a solution with B = 2 or 3 (K = 3 and 96
      need slabs % 3 == 0; a slab then straddles groups and, at B = 3, clouds), rotating C_out, D, the layout and the
      pitches; K = 32 runs at KITTI scale (coordinates ~70, differences ~1e-3).
    test_shapes   at 8 C (one trip) and 8 C + 5 (two trips), K = 32:
        C_out 32, 64  x  D 1, 3, 6, 9  x  xyz_first 0, 1  x  ldx round4(3 + D), 12 (ldx < 12: the dump-slot path of the
        quads beyond the pitch)  x  ldw 3 + D, 3 + D + 5 (values of 1e30 behind the row)  x  ldy C_out, C_out + 8, all with
        stats; stats == NULL on two of the four pitch pairs, Y bit-equal to the run with stats.  D = 3 and 9 at KITTI scale.
    test_refusals   D = 0, D = 10, C_out 48, P % 64 != 0, ldx 16, idx NULL, new_xyz NULL: PN2_EUNSUPPORTED, nothing written.

A too-loose wait corrupts rows only when timing allows it: every problem runs once, nothing loops to provoke it.

Measured on an MI355X (C = 256, so 2047 .. 4097 slabs = 131 008 .. 262 208 rows in the large cases), worst over the runs:
    test_slab_counts   |err| / bound of Y 0.25 .. 0.56 per slab count (1: 0.26, 8C+1: 0.54, m6: 0.56, 16C+1: 0.42);
                       sum y within 6.7e-8 of sum |y|, sum y^2 within 1.2e-7 (small problems), 2.7e-8 / 2.3e-8 (large)
    test_shapes        |err| / bound 0.12 (D = 9, KITTI scale) .. 0.61 (D = 1); sums within 2.4e-8 / 1.9e-8 of their scales
    X bit-equal and Y bit-equal with / without stats in all 288 + 31 runs; no guard element touched.
The fp64 statements are formed on the GPU and the runs of one problem are checked behind one synchronisation: the file
takes 2.8 s (27 tests), the largest single test 0.9 s (the first one: library load).
"""
import pytest
import torch

import fused_ref as R
from pointnet12_amd import _lib

pytestmark = pytest.mark.gpu

PN2_EUNSUPPORTED = -3                    # include/pn2.h
I32 = torch.int32


def _p(t):
    return None if t is None else t.data_ptr()


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _split(slabs, K):
    """(B, S) with B * S * K = 64 * slabs and B = 2 or 3, or None."""
    P = 64 * slabs
    if P % K:
        return None
    G = P // K
    for B in (2, 3):
        if G % B == 0:
            return B, G // B
    return None


def _trips(slabs, C):
    """(fewest, most) trips of a wave and the number of waves that own no slab."""
    waves = 4 * min(-(-slabs // 4), 2 * C)
    per = [-(-(slabs - w) // waves) if w < slabs else 0 for w in (0, waves - 1)]
    return per[1], per[0], max(0, waves - slabs)


def _guard_misses(buf, P, C):
    """Device scalar: elements behind row P or column C that no longer hold the sentinel + elements inside that still do."""
    bits = buf.view(I32)
    return ((bits[P:] != R.SENTINEL).sum() + (bits[:P, C:] != R.SENTINEL).sum() + (bits[:P, :C] == R.SENTINEL).sum()).double()


def _launch(case, xyz_first, ldx, ldy, with_stats):
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    geo, co = case["geo"], case["co"]
    dev = geo["xyz"].device
    P = geo["B"] * geo["S"] * geo["K"]
    Xb, Yb = R.guarded(P, ldx, dev), R.guarded(P, ldy, dev)
    stats = torch.zeros(R.STAT_REPLICAS * 2 * co, device=dev, dtype=torch.float64) if with_stats else None
    rc = lib.pn2_group_conv_fwd(_p(geo["xyz"]), _p(geo["points"]), _p(geo["new_xyz"]), _p(geo["idx"]), geo["B"], geo["N"], geo["S"],
                                geo["K"], geo["D"], int(xyz_first), _p(case["w_store"]), case["ldw"], _p(case["bias"]), _p(Xb), ldx,
                                _p(Yb), ldy, co, _p(stats), stream)
    assert rc == 0, rc
    return Xb, Yb, stats


def _measure(st, Xb, Yb, stats, P, co):
    """[7] on the device: the five numbers of fused_ref.group_conv_errors, the guard misses of X and of Y."""
    sums = None if stats is None else stats.view(R.STAT_REPLICAS, 2, co).sum(0)
    e = R.group_conv_errors(st, Xb[:P], Yb[:P, :co], sums)
    return torch.cat([e, torch.stack([_guard_misses(Xb, P, Xb.shape[1]), _guard_misses(Yb, P, co)])])


def _assert_all(tags, rows):
    """One synchronisation for all runs of a problem; returns the worst (Y err / bound, sum y, sum y^2)."""
    rows = torch.stack(rows).cpu().tolist()
    for tag, e in zip(tags, rows):
        assert e[5] == 0 and e[6] == 0, (tag, "guards: X", e[5], "Y", e[6])
        assert e[0] == 0, (tag, "elements of X not bit-equal to the float32 statement", e[0])
        assert e[1] == 0, (tag, "elements of Y outside the bound", e[1], "worst err / bound", e[2])
        assert R.group_conv_ok(e), (tag, "sum y, sum y^2 relative errors", e[3], e[4])
    return tuple(max(e[i] for e in rows) for i in (2, 3, 4))


SLAB_SPECS = {"1": (0, 1), "3": (0, 3), "4": (0, 4), "5": (0, 5), "8C-1": (8, -1), "8C": (8, 0), "8C+1": (8, 1), "8C+5": (8, 5),
              "m6": None, "16C+1": (16, 1)}
# per K of fused_ref.GROUP_CONV_K = (16, 32, 64, 3, 96): (C_out, D, xyz_first, ldx or 0 for round4(3 + D), ldw extra, ldy extra, kitti)
ROTATION = [(64, 6, 0, 12, 0, 0, False), (32, 3, 1, 0, 5, 8, True), (64, 9, 1, 12, 0, 8, False), (32, 1, 0, 0, 3, 0, False),
            (64, 6, 1, 0, 0, 8, False)]


@pytest.mark.parametrize("spec", list(SLAB_SPECS))
def test_slab_counts(dev, spec):
    """Every trip count of the persistent loop (module docstring), each K that has a solution at this slab count."""
    C = _cus(dev)
    slabs = (8 * C // 6 + 1) * 6 if SLAB_SPECS[spec] is None else SLAB_SPECS[spec][0] * C + SLAB_SPECS[spec][1]
    tags, rows, ran = [], [], []
    for i, K in enumerate(R.GROUP_CONV_K):
        bs = _split(slabs, K)
        if bs is None:
            continue
        B, S = bs
        co, D, xyz_first, ldx, ldw_extra, ldy_extra, kitti = ROTATION[i]
        if spec in ("8C+5", "4"):                                  # (the other C_out on the other counted waits)
            co = 96 - co
        ldx = ldx or R.round4(3 + D)
        case = R.group_conv_case(dev, B, S, K, D, co, 100 * slabs + K, kitti=kitti, ldw_extra=ldw_extra)
        st = R.group_conv_statement(case, xyz_first, ldx)
        Xb, Yb, stats = _launch(case, xyz_first, ldx, co + ldy_extra, True)
        if slabs <= 5:                                             # (the shared helper's own messages, on the small problems)
            torch.cuda.synchronize()
            R.check_guards(Xb, 64 * slabs, ldx, "X", pad_zero=False)
            R.check_guards(Yb, 64 * slabs, co, "Y", pad_zero=False)
        rows.append(_measure(st, Xb, Yb, stats, 64 * slabs, co))
        tags.append((spec, slabs, "B S K", B, S, K, "co D", co, D))
        ran.append(K)
    assert {16, 32} <= set(ran)
    if spec == "m6":
        assert {64, 3, 96} <= set(ran)
    worst = _assert_all(tags, rows)
    print("slabs %s = %d (C = %d): trips %d..%d, %d idle waves, K %s: Y err/bound %.3f  sums %.2e %.2e" %
          ((spec, slabs, C) + _trips(slabs, C) + (ran,) + worst))


@pytest.mark.parametrize("two_trips", [False, True])
@pytest.mark.parametrize("co,D", R.GROUP_CONV_CD)
def test_shapes(dev, co, D, two_trips):
    """C_out x D x xyz_first x ldx x ldw x ldy x stats (module docstring) at 8 C and 8 C + 5 slabs."""
    C = _cus(dev)
    slabs, K = 8 * C + (5 if two_trips else 0), 32
    B, S = _split(slabs, K)
    P, ci = 64 * slabs, 3 + D
    seed = 7 * slabs + 100 * co + D
    cases = [R.group_conv_case(dev, B, S, K, D, co, seed, kitti=D in (3, 9), ldw_extra=x) for x in (0, 5)]
    assert torch.equal(cases[0]["W"], cases[1]["W"]) and torch.equal(cases[0]["bias"], cases[1]["bias"])
    tags, rows, same = [], [], []
    for xyz_first in (0, 1):
        for ldx in sorted({R.round4(ci), 12}):
            st = R.group_conv_statement(cases[0], xyz_first, ldx)
            for wi, case in enumerate(cases):
                for ldy in (co, co + 8):
                    Xb, Yb, stats = _launch(case, xyz_first, ldx, ldy, True)
                    rows.append(_measure(st, Xb, Yb, stats, P, co))
                    tags.append(("xyz_first ldx ldw ldy", xyz_first, ldx, case["ldw"], ldy, "stats"))
                    if (ldy == co) == (wi == 0):
                        Xn, Yn, _ = _launch(case, xyz_first, ldx, ldy, False)
                        rows.append(_measure(st, Xn, Yn, None, P, co))
                        tags.append(("xyz_first ldx ldw ldy", xyz_first, ldx, case["ldw"], ldy, "stats NULL"))
                        same.append((Yn.view(I32) != Yb.view(I32)).sum())
    worst = _assert_all(tags, rows)
    assert int(torch.stack(same).sum()) == 0, "Y differs between stats given and stats == NULL"
    print("shapes C_out %d D %d, %d slabs, %d runs: Y err/bound %.3f  sums %.2e %.2e" % ((co, D, slabs, len(rows)) + worst))


def test_refusals(dev):
    """What the kernel cannot do is refused with PN2_EUNSUPPORTED before anything is launched: X and Y keep the sentinel."""
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    N = 16

    def attempt(what, B=2, S=8, K=16, D=3, co=32, ldx=None, idx=True, new=True):
        geo = R.draw_geometry(dev, B, N, S, K, max(D, 1), 5)
        ci = 3 + D
        ldx = ldx or R.round4(ci)
        W = torch.randn(co, ci, device=dev)
        bias = torch.randn(co, device=dev)
        P = B * S * K
        Xb, Yb = R.guarded(P, ldx, dev), R.guarded(P, co, dev)
        stats = torch.zeros(R.STAT_REPLICAS * 2 * co, device=dev, dtype=torch.float64)
        rc = lib.pn2_group_conv_fwd(_p(geo["xyz"]), _p(geo["points"]) if D else None, _p(geo["new_xyz"]) if new else None,
                                    _p(geo["idx"]) if idx else None, B, N, S, K, D, 1, _p(W), ci, _p(bias), _p(Xb), ldx, _p(Yb), co, co,
                                    _p(stats), stream)
        assert rc == PN2_EUNSUPPORTED, (what, rc)
        return what, ((Xb.view(I32) != R.SENTINEL).sum() + (Yb.view(I32) != R.SENTINEL).sum() + (stats != 0).sum())

    left = [attempt("D = 0", D=0), attempt("D = 10", D=10), attempt("C_out 48", co=48), attempt("P % 64 != 0", K=15),
            attempt("ldx 16", ldx=16), attempt("idx NULL", idx=False), attempt("new_xyz NULL", new=False)]
    written = torch.stack([w for _, w in left]).cpu().tolist()
    for (what, _), w in zip(left, written):
        assert w == 0, (what, "elements written by a refused call", w)
