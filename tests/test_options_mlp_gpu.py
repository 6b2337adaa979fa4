"""GPU: the kernels the GEMM dispatch options route to (PN2_OPTION_LIST of csrc/pn2_common.h; the ledger of
tests/options_ref.py says which test covers which option), kernel-level through the C ABI on the fixed operands of
tests/mlp_ref.py, against fp64.

include/pn2.h states that an option changes results by fp32 summation order at most.  Most options route a call to another
template instantiation that the library ships and that no default-route test reaches.  Every case here runs the entry point
twice on the SAME operands -- once with the options of its base route, once with the option under test -- and

  * asserts through pn2_last_kernel() that the second call launched a DIFFERENT instantiation (template arguments included)
    and, where the dispatch code names it, which one.  A case whose route did not change fails.  Options that change only
    the grid of the same instantiation (options_ref.NOTE_GRID) assert that the name did NOT change instead;
  * holds BOTH results to fp64 with the bounds tests/test_mlp_seams_gpu.py states for that entry point on this operand
    generator (none of them new, none fitted to a result): Y, and dX / dW / db of a layer without an input BatchNorm block,
    within 2e-6 max|ref| max(1, sqrt(n) / 8), n the contraction length; sum y and sum y^2 within 1e-5 of sum |y| and sum y^2;
    dX, dW and the two reductions of a BatchNorm layer within 3e-6 of the tensor's largest entry.  The option route gets the
    bound of the default route, not a looser one;
  * checks the guard rows / columns of Y and dX and the frame of dW / dbias (mlp_ref: GUARDS), and scales the rows behind
    the last whole tile by 32 where the route has a streamed tail (mlp_ref: SEAM-SENSITIVE INPUTS).

Shapes are the smallest that reach each branch; what depends on the CU count is computed from the device, and every case
asserts the dispatch condition it relies on.  The measured errors of both routes are printed (-s).
"""
import re

import pytest
import torch

from pointnet12_amd import _lib

import mlp_ref as R
import options_ref as O
from options_ref import options
import test_mlp_seams_gpu as S

pytestmark = pytest.mark.gpu


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _cdiv(a, b):
    return -(-a // b)


def _inst(name):
    """`kernel<template arguments>` of a demangled kernel name (without the namespace and the parameter list)."""
    m = re.search(r"(\w+)<", name)
    assert m, "no kernel recorded: %r" % name
    i, depth = m.end(), 1
    while depth:
        depth += (name[i] == "<") - (name[i] == ">")
        i += 1
    return name[m.start():i].replace("(anonymous namespace)::", "")


def _fmt(errs):
    return "  ".join("%s %.2e/%.1e" % (k, e, tol) for k, (e, tol) in errs.items())


def _ab(what, run, base, alt, expect=None, base_expect=None, grid_only=False):
    """run() -> (kernel name, {label: (error, bound)}) under `base` and under `base` + `alt`: prints both, asserts the route
    (changed, and to `expect`; unchanged where grid_only) and then every bound of both runs."""
    with options(**base):
        n0, e0 = run()
    with options(**dict(base, **alt)):
        n1, e1 = run()
    i0, i1 = _inst(n0), _inst(n1)
    print("%s\n    base %s: %s  [%s]\n    with %s: %s  [%s]" % (what, base or "defaults", _fmt(e0), i0[:110], alt, _fmt(e1), i1[:110]))
    if base_expect:
        assert re.search(base_expect, i0), (what, "base route", base_expect, i0)
    if grid_only:
        assert i0 == i1, (what, "the option was expected to change the grid only", i0, i1)
    else:
        assert i0 != i1, (what, "the option did not change the route", alt, i0)
        if expect:
            assert re.search(expect, i1), (what, expect, i1)
    for tag, errs in (("base", e0), ("option", e1)):
        for k, (e, tol) in errs.items():
            assert e <= tol, (what, tag, k, e, tol)
    return e0, e1


def _plain_tol(n):
    return 2e-6 * max(1.0, n ** 0.5 / 8)


BN_TOL = 3e-6


# =============================================================================================== runs on fixed operands

def _fwd_run(dev, P, K, N, affine, seed, tail_from=None):
    """pn2_conv1x1_fwd with stats on one operand set; run(rows) takes the leading `rows` rows."""
    lib = _lib.load()
    c, ref = R.fixed_forward_case(dev, P, K, N, seed, affine=affine, ldy=R.round4(N) + (0 if affine else 8), tail_from=tail_from)

    def run(rows=P):
        Yb, stats = R.guarded(rows, c["ldy"], dev), torch.zeros(R.STAT_REPLICAS * 2 * N, device=dev, dtype=torch.float64)
        name = S._fwd(lib, c, Yb, rows, K, N, stats)
        _, e_s1, e_s2 = S._check_fwd(dev, Yb, stats, ref, 0, rows, K, N, "Y")
        head = tail_from if (tail_from is not None and tail_from < rows) else rows
        e_y = max(S._parts(Yb[:rows, :N], ref["Y"][:rows], head))
        return name, {"Y": (e_y, S._y_tol(K)), "sum y": (e_s1, 1e-5), "sum y^2": (e_s2, 1e-5)}
    return run


def _layer_run(dev, kind, P, co, ci, Kp, seed, masked=True, tail_from=None, dbias=False):
    """pn2_conv1x1_dgrad / _wgrad / _bwd / _bwd_pair of one layer on one operand set; run(rows) takes the leading rows."""
    lib = _lib.load()
    c, ref = R.fixed_layer_case(dev, P, co, ci, Kp, seed, masked=masked, tail_from=tail_from)
    g = torch.Generator(device=dev).manual_seed(seed + 17)
    rnd = lambda *s_: torch.randn(*s_, device=dev, generator=g)

    def run(rows=P):
        o = S._bwd_outputs(dev, c, rows, co, ci, seed + 3, wide=True)
        head = tail_from if (tail_from is not None and tail_from < rows) else rows
        tol_x = BN_TOL if masked else _plain_tol(co)
        tol_w = BN_TOL if masked else _plain_tol(rows)
        if kind == "wgrad":
            db, db0 = R.framed(1, co, co + 4, rnd) if dbias else (None, None)
            name = S._wgrad(lib, c, o, rows, co, ci, dbias=db)
            torch.cuda.synchronize()
            sums = ref["part"](0, rows)
            R.check_frame(o["dW"], o["dW0"], co, ci, "dW")
            errs = {"dW": (R.rel(o["dW"][:co, :ci], o["dW0"][:co, :ci].double() + sums["dW"]), tol_w)}
            if dbias:
                R.check_frame(db, db0, 1, co, "dbias")
                errs["db"] = (R.rel(db[0, :co], db0[0, :co].double() + sums["db"]), tol_w)
            assert bool((o["dX"].view(torch.int32) == R.SENTINEL).all()), "the weight gradient wrote into dX"
            return name, errs
        if kind == "dgrad":
            name = S._dgrad(lib, c, o, rows, co, ci)
        elif kind == "bwd":
            name = S._bwd(lib, c, o, rows, co, ci)
        else:
            assert kind in ("pair", "split")               # pn2_conv1x1_bwd_pair: X = the layer's input = prev_Y
            rc = lib.pn2_conv1x1_bwd_pair(*c["dz_args"], c["Y"].data_ptr(), c["ldc"], c["coef"].data_ptr(), c["W"].data_ptr(), c["ldw"],
                                          c["Yp"].data_ptr() if masked else None, c["ldp"], S._p(c["affp"]), o["dX"].data_ptr(), o["ldxo"],
                                          S._p(o["red"]), c["Yp"].data_ptr(), c["ldp"], S._p(c["affp"]), o["dW"].data_ptr(), o["lddw"],
                                          rows, co, ci, None, S._stream())
            assert rc in (0, _lib.PN2_OK_SPLIT), rc
            name = S._last(lib) + (" [rc %d]" % rc)
        e = S._check_bwd(o, ref, rows, co, ci, head, kind, dW=kind != "dgrad")
        n_x = 2 if head < rows else 1
        errs = {"dX": (max(e[:n_x]), tol_x)}
        rest = list(e[n_x:])
        if kind != "dgrad":
            errs["dW"] = (rest.pop(0), tol_w)
        if masked:
            errs["red0"], errs["red1"] = (rest[0], BN_TOL), (rest[1], BN_TOL)
        return name, errs
    return run


# =============================================================================================== (1) few-row NT

NT_OFF = {"PN2_FEWROW_MAX_TILES": 0, "PN2_FEWROW_MAX_TILES_DGRAD": 0}
NT_CASES = [
    # id, rows, base options, option under test, the instantiation the dispatch code names (dispatch_nt_vec, launch_fewrow)
    ("fewrow-off", "P32", {}, NT_OFF, r"^gemm_nt_kernel<32, 64, 32, 1, 2, \d, 1, ", r"^fewrow_nt_kernel<4, "),
    ("fewrow-ks1", "P32", {}, {"PN2_FEWROW_KS": 1}, r"^fewrow_nt_kernel<1, ", r"^fewrow_nt_kernel<4, "),
    ("fewrow-ks2", "P32", {}, {"PN2_FEWROW_KS": 2}, r"^fewrow_nt_kernel<2, ", r"^fewrow_nt_kernel<4, "),
    ("depth2", "P32", NT_OFF, {"PN2_NT_SMALL_DEPTH": 2}, r"^gemm_nt_kernel<32, 64, 32, 1, 2, 2, 3, ", r"^gemm_nt_kernel<32, 64, 32, 1, 2, \d, 1, "),
    ("depth3", "P32", NT_OFF, {"PN2_NT_SMALL_DEPTH": 3}, r"^gemm_nt_kernel<32, 64, 32, 1, 2, 2, 1, .*, 4, false>$", None),
    ("depth4", "P32", NT_OFF, {"PN2_NT_SMALL_DEPTH": 4}, r"^gemm_nt_kernel<32, 64, 32, 1, 2, 2, 1, .*, 1, true>$", None),
    ("depth2-ragged", "P32-27", {}, {"PN2_NT_SMALL_DEPTH": 2}, r"^gemm_nt_kernel<32, 64, 32, 1, 2, 2, 3, ", None),
    ("depth3-ragged", "P32-27", {}, {"PN2_NT_SMALL_DEPTH": 3}, r"^gemm_nt_kernel<32, 64, 32, 1, 2, 2, 1, .*, 4, false>$", None),
    ("depth4-ragged", "P32-27", {}, {"PN2_NT_SMALL_DEPTH": 4}, r"^gemm_nt_kernel<32, 64, 32, 1, 2, 2, 1, .*, 1, true>$", None),
    ("depth4-64x64", "P64", NT_OFF, {"PN2_NT_SMALL_DEPTH": 4}, r"^gemm_nt_kernel<64, 64, 32, 2, 2, 2, 1, .*, 1, true>$", r"^gemm_nt_kernel<64, 64, 32, 2, 2, \d, 1, "),
    ("depth4-64x64-ragged", "P64-27", {}, {"PN2_NT_SMALL_DEPTH": 4}, r"^gemm_nt_kernel<64, 64, 32, 2, 2, 2, 1, .*, 1, true>$", None),
    ("cfg7", "P32", NT_OFF, {"PN2_NT_CFG": 7}, r"^gemm_nt_kernel<64, 128, 16, 2, 2, ", None),
    ("cfg8", "P32", NT_OFF, {"PN2_NT_CFG": 8}, r"^gemm_nt_kernel<64, 64, 32, 2, 2, ", None),
    ("cfg7-64x64", "P64", NT_OFF, {"PN2_NT_CFG": 7}, r"^gemm_nt_kernel<64, 128, 16, 2, 2, ", None),
    ("cfg7-ragged", "P32-27", {}, {"PN2_NT_CFG": 7}, r"^gemm_nt_kernel<64, 128, 16, 2, 2, ", None),
    ("cfg8-ragged", "P32-27", {}, {"PN2_NT_CFG": 8}, r"^gemm_nt_kernel<64, 64, 32, 2, 2, ", None),
]


@pytest.mark.parametrize("rows,base,alt,expect,base_expect", [pytest.param(*c[1:], id=c[0]) for c in NT_CASES])
def test_few_row_nt_options_forward_and_data_gradient(dev, rows, base, alt, expect, base_expect):
    """dispatch_nt_vec / launch_fewrow of csrc/mlp.hip on 512 -> 256 (forward: K = 512, N = 256; data gradient: C_out = 512,
    C_in = 256), each with a BatchNorm block and plain.  P32 rows (1024 on 256 CUs) have few enough 64 x 64 tiles for the
    32 x 64 small tile, P64 (3072) only for the 64 x 64 one; both are multiples of 32 with a tile count that is a multiple of
    4, so fewrow_nt_kernel takes them by default (four waves per tile) and FEWROW_MAX_TILES = FEWROW_MAX_TILES_DGRAD = 0 is
    the base route of the cases about the tiles behind it.  The -27 row counts are no multiple of 32: fewrow_nt_kernel never
    takes them, and the last tile of every instantiation is ragged."""
    cu = _cus()
    P32, P64 = 64 * max(1, cu // 16), 64 * (3 * cu // 16)
    P = {"P32": P32, "P64": P64}[rows.split("-")[0]] - (27 if rows.endswith("-27") else 0)
    K, N = 512, 256
    # the dispatch conditions this case relies on (dispatch_nt_vec, launch_fewrow)
    t64 = _cdiv(P, 64)
    if rows.startswith("P32"):
        assert t64 * _cdiv(N, 64) * 2 <= cu
    else:
        assert t64 * _cdiv(N, 64) * 2 > cu and t64 * _cdiv(N, 128) * 2 <= cu
    if P % 32 == 0:
        tiles = (P // 32) * (N // 64)
        assert tiles % 4 == 0 and tiles <= 512                                  # fewrow_nt_kernel takes it by default
        assert not rows.startswith("P32") or tiles * 4 <= 4 * cu                # ... with four waves per tile
    for affine in (True, False):
        what = "NT %s fwd %d x %d -> %d (%s)" % (rows, P, K, N, "bn" if affine else "plain")
        _ab(what, _fwd_run(dev, P, K, N, affine, 100 + P + affine), base, alt, expect, base_expect)
    for masked in (True, False):
        what = "NT %s dgrad %d x %d -> %d (%s)" % (rows, P, K, N, "bn" if masked else "plain")
        _ab(what, _layer_run(dev, "dgrad", P, K, N, 0, 200 + P + masked, masked=masked), base, alt, expect, base_expect)


@pytest.mark.parametrize("K", [64, 128])
def test_nt_cfg_9_sends_96_columns_to_the_128_wide_tile(dev, K):
    """NT_CFG = 9: K -> 96 leaves the exact 128 x 96 tile for the 64 x 128 one (25 % padding columns), at a row count with too
    many tiles for the few-row branches and a ragged last tile."""
    cu = _cus()
    P = 64 * (cu // 2 + 1) + 37
    assert _cdiv(P, 64) * _cdiv(96, 128) * 2 > cu and P < _lib.options()["PN2_RES_MIN_ROWS"]
    alt = {"PN2_NT_CFG": 9}
    for affine in (True, False):
        _ab("NT_CFG=9 fwd %d x %d -> 96 (%s)" % (P, K, "bn" if affine else "plain"), _fwd_run(dev, P, K, 96, affine, 300 + K + affine), {}, alt,
            r"^gemm_nt_kernel<64, 128, 16, 2, 2, ", r"^gemm_nt_kernel<128, 96, 16, 4, 1, ")
    for masked in (True, False):
        _ab("NT_CFG=9 dgrad %d x %d -> 96 (%s)" % (P, K, "bn" if masked else "plain"), _layer_run(dev, "dgrad", P, K, 96, 0, 310 + K + masked, masked=masked),
            {}, alt, r"^gemm_nt_kernel<64, 128, 16, 2, 2, ", r"^gemm_nt_kernel<128, 96, 16, 4, 1, ")


@pytest.mark.parametrize("K", [128, 256])
def test_nt_nsplit_off_runs_196_columns_in_one_launch(dev, K):
    """NT_NSPLIT = 0: 196 output columns as ONE launch of 64 x 128 tiles (the second column tile 47 % padding) instead of 128
    columns + a 96-wide remainder launch; the default's last launch is the remainder's 128 x 96 tile."""
    cu = _cus()
    P = max(4096, 64 * (cu // 4)) + 37
    assert _cdiv(P, 64) * _cdiv(196, 128) * 2 > cu and P < _lib.options()["PN2_WIDE_MIN_ROWS"]
    alt = {"PN2_NT_NSPLIT": 0}
    for affine in (True, False):
        _ab("NT_NSPLIT=0 fwd %d x %d -> 196 (%s)" % (P, K, "bn" if affine else "plain"), _fwd_run(dev, P, K, 196, affine, 400 + K + affine), {}, alt,
            r"^gemm_nt_kernel<64, 128, 16, 2, 2, ", r"^gemm_nt_kernel<128, 96, 16, 4, 1, ")
    _ab("NT_NSPLIT=0 dgrad %d x %d -> 196 (bn)" % (P, K), _layer_run(dev, "dgrad", P, K, 196, 0, 410 + K), {}, alt,
        r"^gemm_nt_kernel<64, 128, 16, 2, 2, ", r"^gemm_nt_kernel<128, 96, 16, 4, 1, ")


# =============================================================================================== (2) TN

TN_CASES = [
    # id, C_out, C_in, rows, option under test, expected instantiation (dispatch_tn), grid only
    ("narrow0-32x32", 32, 32, 8192 + 5, {"PN2_TN_NARROW": 0}, r"^gemm_tn_kernel<128, 32, 32, 4, 1, 2, ", r"^gemm_tn_kernel<32, 32, 64, 1, 1, \d, .*, 4, 1, 1>$", False),
    ("narrow0-64x32", 64, 32, 8192 + 5, {"PN2_TN_NARROW": 0}, r"^gemm_tn_kernel<128, 32, 32, 4, 1, 2, ", r"^gemm_tn_kernel<64, 32, 32, 2, 1, \d, .*, 2, 1, 1>$", False),
    ("depth1-128x128", 128, 128, 4096, {"PN2_TN_SMALL_DEPTH": 1}, r"^gemm_tn_kernel<64, 64, 32, 2, 2, 2, .*, 1, 1, 1>$", r"^gemm_tn_kernel<64, 64, 32, 2, 2, 2, .*, 1, 2, 4>$", False),
    ("depth3-128x128", 128, 128, 4096, {"PN2_TN_SMALL_DEPTH": 3}, r"^gemm_tn_kernel<64, 64, 32, 2, 2, 2, .*, 1, 2, 1>$", None, False),
    ("smallp0-128x128", 128, 128, 4096 + 5, {"PN2_TN_SMALLP": 0}, r"^gemm_tn_kernel<128, 128, 16, 2, 2, 2, ", None, False),
    ("smallp0-128x64", 128, 64, 4096 + 5, {"PN2_TN_SMALLP": 0}, r"^gemm_tn_kernel<128, 64, 32, 2, 2, 2, ", None, False),
    ("smallp0-64x128", 64, 128, 4096 + 5, {"PN2_TN_SMALLP": 0}, r"^gemm_tn_kernel<64, 128, 32, 2, 2, 2, ", None, False),
    ("cfg3-128x128", 128, 128, 4096 + 5, {"PN2_TN_CFG": 3}, r"^gemm_tn_kernel<128, 128, 16, 2, 2, 2, ", None, False),
    ("cfg1-128x64", 128, 64, 131072 + 5, {"PN2_TN_CFG": 1}, r"^gemm_tn_kernel<128, 64, 32, 2, 2, 2, ", r"^gemm_tn_kernel<128, 64, 16, 2, 2, 3, ", False),
    ("cfg1-64x128", 64, 128, 131072 + 5, {"PN2_TN_CFG": 1}, r"^gemm_tn_kernel<64, 128, 32, 2, 2, 2, ", r"^gemm_tn_kernel<64, 128, 16, 2, 2, \d, ", False),
    ("splitdiv2-128x128", 128, 128, 4096 + 5, {"PN2_TN_SPLITDIV": 2}, None, None, True),
    ("splitdiv8-128x128", 128, 128, 4096 + 5, {"PN2_TN_SPLITDIV": 8}, None, None, True),
    ("splitdiv8-large-tiles", 128, 128, 4096 + 5, {"PN2_TN_SMALLP": 0, "PN2_TN_SPLITDIV": 8}, r"^gemm_tn_kernel<128, 128, 16, 2, 2, 2, ", None, False),
]


@pytest.mark.parametrize("co,ci,P,alt,expect,base_expect,grid_only", [pytest.param(*c[1:], id=c[0]) for c in TN_CASES])
def test_tn_options_on_the_streamed_weight_gradient(dev, co, ci, P, alt, expect, base_expect, grid_only):
    """dispatch_tn / launch_tn of csrc/mlp.hip through pn2_conv1x1_wgrad, with the layer input behind a BatchNorm block and
    as stored: TN_NARROW = 0 (the narrow sa1 products on the general 128 x 32 tile), TN_SMALL_DEPTH 1 and 3 (the few-row
    64 x 64 tile with one stage in flight / one accumulator set), TN_SMALLP = 0 and TN_CFG = 3 (the large-P tile
    configurations at a size where fp64 is instant), TN_CFG = 1 (the 32-deep large tiles above 131 072 rows, where the
    default is 16-deep), TN_SPLITDIV 2 and 8 (a shallower split over P: grid only)."""
    assert P < _lib.options()["PN2_WIDE_WGRAD_MIN_ROWS"] or (co, ci) not in ((256, 196), (256, 128), (196, 128))
    for masked in (True, False):
        if ci <= 16 and not masked:
            continue
        what = "TN %d x %d, %d rows (%s)" % (co, ci, P, "bn" if masked else "plain")
        _ab(what, _layer_run(dev, "wgrad", P, co, ci, 0, 500 + co + ci + masked, masked=masked), {}, alt, expect, base_expect, grid_only)


@pytest.mark.parametrize("ci", [3, 9, 12])
def test_first_layer_weight_gradient_without_the_skinny_kernel(dev, ci):
    """WGRAD_SKINNY = 0: the first layers' weight gradient (C_in <= 16, no input BatchNorm, P >= 4096) through gemm_tn_kernel's
    narrow tile instead of wgrad_skinny_kernel, at 4096 rows and 4096 + 5, with and without dbias."""
    co = 64
    for P in (4096, 4096 + 5):
        for dbias in (False, True):
            what = "WGRAD_SKINNY=0 %d x %d, %d rows%s" % (co, ci, P, ", dbias" if dbias else "")
            _ab(what, _layer_run(dev, "wgrad", P, co, ci, 0, 600 + ci + P, masked=False, dbias=dbias), {}, {"PN2_WGRAD_SKINNY": 0},
                r"^gemm_tn_kernel<64, 32, 32, 2, 1, ", r"^wgrad_skinny_kernel<%d>$" % ((ci + 3) // 4))


def test_closed_form_first_layer_weight_gradient_workgroups_per_cu(dev):
    """CF_WGS_PER_CU 1 and 4 against the default 2 on pn2_conv1x1_wgrad_cf (16 x 12): the option caps the grid at that many
    workgroups per CU and a workgroup takes 512 rows per trip, so the three settings differ from 2 x 512 x CUs rows on --
    the smallest row count at which the option does anything, plus a ragged 517.  Grid only: same instantiation.  dW (a first
    layer: no input BatchNorm) is held to 2e-6 max|ref| max(1, sqrt(P) / 8) like every plain layer's."""
    lib, cu = _lib.load(), _cus()
    M, N = 16, 12
    P = 2 * 512 * cu + 517
    assert _cdiv(P, 512) > 2 * cu
    g = torch.Generator(device=dev).manual_seed(77)
    rnd = lambda *s_: torch.randn(*s_, device=dev, generator=g)
    dZ, X = rnd(P, M), rnd(P, N) * 1.5 + 0.3
    W, b = rnd(M, N) * 0.3, rnd(M) * 0.1
    coef = R.draw_coef(rnd, M, M, dev)
    c0, q1, q0, mu = (coef[i * M:(i + 1) * M].double() for i in range(4))
    x = X.double()
    Sxx, sx = x.t() @ x, x.sum(0)
    ref = c0[:, None] * (dZ.double().t() @ x) + q1[:, None] * (W.double() @ Sxx + (b.double() - mu)[:, None] * sx[None, :]) + q0[:, None] * sx[None, :]

    def run():
        dW, dW0 = R.framed(M, N, 16, rnd)
        scratch = torch.zeros(int(lib.pn2_conv1x1_wgrad_cf_scratch_bytes()), device=dev, dtype=torch.uint8)
        rc = lib.pn2_conv1x1_wgrad_cf(dZ.data_ptr(), M, coef.data_ptr(), X.data_ptr(), N, W.data_ptr(), N, b.data_ptr(), scratch.data_ptr(), dW.data_ptr(), 16,
                                      P, M, N, None, S._stream())
        assert rc == 0, rc
        name = S._last(lib)
        torch.cuda.synchronize()
        R.check_frame(dW, dW0, M, N, "dW")
        return name, {"dW": (R.rel(dW[:M, :N], dW0[:M, :N].double() + ref), _plain_tol(P))}
    for per_cu in (1, 4):
        _ab("CF_WGS_PER_CU=%d, %d x %d, %d rows" % (per_cu, M, N, P), run, {}, {"PN2_CF_WGS_PER_CU": per_cu}, grid_only=True,
            base_expect=r"^wgrad_first_cf_kernel<1, 8>$")


@pytest.mark.parametrize("masked", [True, False])
def test_bwd_pair_in_one_launch_and_in_two_vs_fp64(dev, masked):
    """BWD_PAIR 0 against 1 on pn2_conv1x1_bwd_pair (128 x 128, a row count that reaches the 64 x 128 leaf of dispatch_nt_vec
    with a ragged last tile): one bwd_pair_kernel launch (return code 0) against pn2_conv1x1_dgrad + pn2_conv1x1_wgrad
    (PN2_OK_SPLIT), BOTH held to fp64 -- dX, dW and the reductions within 3e-6 with the input BatchNorm, within the plain
    layers' bound without."""
    cu = _cus()
    P = 64 * (cu // 2 + 1) + 37
    o = _lib.options()
    assert _cdiv(P, 64) * 2 > cu and P <= o["PN2_TN_SMALLP"] and P < o["PN2_WIDE_MIN_ROWS"]
    run = _layer_run(dev, "pair", P, 128, 128, 0, 700 + masked, masked=masked)
    with options(PN2_BWD_PAIR=1):
        n1, e1 = run()
    with options(PN2_BWD_PAIR=0):
        n0, e0 = run()
    print("bwd_pair 128 x 128, %d rows (%s)\n    one launch: %s  [%s]\n    two: %s  [%s]" % (P, "bn" if masked else "plain", _fmt(e1), n1[-90:], _fmt(e0), n0[-90:]))
    assert re.search(r"bwd_pair_kernel<64, 128, 16, 2, 2, ", n1) and n1.endswith("[rc 0]"), n1
    assert re.search(r"gemm_tn_kernel<64, 64, 32, 2, 2, 2, ", n0) and n0.endswith("[rc %d]" % _lib.PN2_OK_SPLIT), n0
    for errs in (e1, e0):
        for k, (e, tol) in errs.items():
            assert e <= tol, (k, e, tol)


# =============================================================================================== (3) wide and resident families

WIDE_CASES = [
    # id, entry point, C_out (forward: K), C_in (forward: N), Kpool, threshold, rows behind it, tile rows, base, option, base family, option family
    ("wide0-fwd-128x256", "fwd", 128, 256, 0, "Wd", 37, 64, {}, {"PN2_WIDE": 0}, r"^split_nt_kernel<", r"^gemm_nt_kernel<"),
    ("wide0-fwd-128x196", "fwd", 128, 196, 0, "Wd", 37, 64, {}, {"PN2_WIDE": 0}, r"^split_nt_kernel<", r"^gemm_nt_kernel<"),
    ("wide0-fwd-196x256", "fwd", 196, 256, 0, "Wd", 37, 64, {}, {"PN2_WIDE": 0}, r"^split_nt_kernel<", r"^gemm_nt_kernel<"),
    ("res0-fwd-64x64", "fwd", 64, 64, 0, "R", 21, 32, {}, {"PN2_RES": 0}, r"^fwd_res_kernel<", r"^gemm_nt_kernel<"),
    ("wide0-dgrad-196x128", "dgrad", 196, 128, 0, "Wd", 37, 64, {}, {"PN2_WIDE": 0}, r"^split_nt_kernel<", r"^gemm_nt_kernel<"),
    ("wide0-dgrad-256x128-pool64", "dgrad", 256, 128, 64, "Wd", 64, 64, {}, {"PN2_WIDE": 0}, r"^split_nt_kernel<", r"^gemm_nt_kernel<"),
    ("wide0-dgrad-256x196-pool128", "dgrad", 256, 196, 128, "Wd", 128, 64, {}, {"PN2_WIDE": 0}, r"^split_nt_kernel<", r"^gemm_nt_kernel<"),
    ("wide0-wgrad-256x196-pool128", "wgrad", 256, 196, 128, "G", 128, 0, {}, {"PN2_WIDE": 0}, r"^split_tn_kernel<", r"^gemm_tn_kernel<"),
    ("adb196-0-dgrad-196x128", "dgrad", 196, 128, 0, "Wd", 37, 128, {"PN2_SPLIT": 0}, {"PN2_WIDE_ADB196": 0}, r"^regw_nt_kernel<", r"^regw_nt_kernel<"),
    ("k256-0-dgrad-256x196-pool128", "dgrad", 256, 196, 128, "Wd", 128, 64, {}, {"PN2_SPLIT_K256": 0}, r"^split_nt_kernel<", r"^regw_nt_kernel<"),
    ("k256-0-dgrad-256x128-pool64", "dgrad", 256, 128, 64, "Wd", 64, 64, {}, {"PN2_SPLIT_K256": 0}, r"^split_nt_kernel<", r"^regw_nt_kernel<"),
    ("widewgrad0-196x128", "wgrad", 196, 128, 0, "G", 32, 0, {}, {"PN2_WIDE_WGRAD": 0}, r"^split_tn_kernel<", r"^gemm_tn_kernel<"),
    ("splitwgrad0-196x128", "wgrad", 196, 128, 0, "G", 32, 0, {}, {"PN2_SPLIT_WGRAD": 0}, r"^split_tn_kernel<", r"^wgrad_full_kernel<"),
    ("splitwgrad0-256x128-pool64", "wgrad", 256, 128, 64, "G", 64, 0, {}, {"PN2_SPLIT_WGRAD": 0}, r"^split_tn_kernel<", r"^wgrad_full_kernel<"),
    ("splitwgrad0-256x196-pool128", "wgrad", 256, 196, 128, "G", 128, 0, {}, {"PN2_SPLIT_WGRAD": 0}, r"^split_tn_kernel<", r"^wgrad_full_kernel<"),
    ("splitres2-bwd-32x32", "bwd", 32, 32, 0, "R", 37, 64, {}, {"PN2_SPLIT_RES": 2}, r"^bwd_res_kernel<", r"^split_bwd_res_kernel<"),
    ("splitres2-bwd-64x32-pool32", "bwd", 64, 32, 32, "R", 32, 64, {}, {"PN2_SPLIT_RES": 2}, r"^bwd_res_kernel<", r"^split_bwd_res_kernel<"),
]


@pytest.mark.parametrize("entry,co,ci,Kp,thr,behind,tile,base,alt,base_family,alt_family", [pytest.param(*c[1:], id=c[0]) for c in WIDE_CASES])
def test_wide_and_resident_options_at_their_row_thresholds(dev, entry, co, ci, Kp, thr, behind, tile, base, alt, base_family, alt_family):
    """The switches of csrc/mlp_wide.hip and csrc/mlp_res.hip on the layer shapes their branches name, at the row threshold
    read from the library plus a few rows: WIDE = 0 and, on the forward, RES = 0 (the streamed kernels take the whole call),
    WIDE_ADB196 = 0 (the second fp32 196 -> 128 data-gradient instantiation; SPLIT = 0 is its base route), SPLIT_K256 = 0 (the pooled
    C_out = 256 data gradients on the fp32 register-stationary kernel), WIDE_WGRAD = 0 and SPLIT_WGRAD = 0 (streamed /
    fp32 full-tile weight gradients), SPLIT_RES = 2 (the 32 x 32 and pooled 64 x 32 fused pairs on the bf16 pipe).
    Where the entry point hands a ragged remainder to the streamed kernels, the whole tiles run ALONE first -- that call's
    kernel name is what the option must change -- and then the ragged call, whose tail rows are scaled by 32."""
    P = S._thr(thr) + behind
    head = P if tile == 0 else (P // tile) * tile
    seed = 800 + co + ci + Kp
    tail_from = head if head < P else None
    if entry == "fwd":
        run = _fwd_run(dev, P, co, ci, True, seed, tail_from=tail_from)
        what = "%s %d -> %d" % (entry, co, ci)
    else:
        run = _layer_run(dev, entry, P, co, ci, Kp, seed, tail_from=tail_from)
        what = "%s %d x %d, K=%d" % (entry, co, ci, Kp)
    if head < P:
        _ab("%s, %d whole-tile rows alone" % (what, head), lambda: run(head), base, alt, alt_family, base_family)
        with options(**base):
            n0, e0 = run()
        with options(**dict(base, **alt)):
            n1, e1 = run()
        print("%s, P = %d = %d + %d\n    base: %s  [%s]\n    with %s: %s  [%s]" % (what, P, head, P - head, _fmt(e0), _inst(n0)[:80], alt, _fmt(e1), _inst(n1)[:80]))
        assert S._streamed(n0) and S._streamed(n1), (n0, n1)               # the tail's launch
        for errs in (e0, e1):
            for k, (e, tol) in errs.items():
                assert e <= tol, (what, k, e, tol)
    else:
        _ab("%s, %d rows" % (what, P), run, base, alt, alt_family, base_family)


def test_res_off_hands_the_fused_backward_to_the_streamed_pair(dev):
    """RES = 0 on the backward.  pn2_conv1x1_bwd itself does not read the option: its caller asks pn2_bwd_res_supported()
    (pointnet_util does) and runs pn2_conv1x1_dgrad + pn2_conv1x1_wgrad where the answer is 0.  So: both support queries
    answer 1 by default and 0 with RES = 0 for 64 x 64 at RES_MIN_ROWS + 37 rows, and the fused call (default) and the
    streamed pair (RES = 0) on the same operands each meet the BatchNorm layers' 3e-6."""
    lib = _lib.load()
    co = ci = 64
    P = S._thr("R") + 37
    head = (P // 64) * 64
    runs = {k: _layer_run(dev, k, P, co, ci, 0, 850, tail_from=head) for k in ("bwd", "dgrad", "wgrad")}
    assert lib.pn2_res_supported(P, co, ci) == 1 and lib.pn2_bwd_res_supported(P, co, ci, 0, 1) == 1
    n_f, e_f = runs["bwd"](head)
    assert S._is(n_f, "split_bwd_res_kernel"), n_f
    n_r, e_r = runs["bwd"]()
    with options(PN2_RES=0):
        assert lib.pn2_res_supported(P, co, ci) == 0 and lib.pn2_bwd_res_supported(P, co, ci, 0, 1) == 0
        n_d, e_d = runs["dgrad"]()
        n_w, e_w = runs["wgrad"]()
    print("bwd 64 x 64, P = %d = %d + %d\n    fused, whole tiles alone: %s  [%s]\n    fused + tail: %s  [%s]\n    RES=0, dgrad: %s  [%s]\n    RES=0, wgrad: %s  [%s]" %
          (P, head, P - head, _fmt(e_f), _inst(n_f)[:60], _fmt(e_r), _inst(n_r)[:60], _fmt(e_d), _inst(n_d)[:60], _fmt(e_w), _inst(n_w)[:60]))
    assert S._is(n_d, "gemm_nt_kernel") and S._is(n_w, "gemm_tn_kernel"), (n_d, n_w)
    for errs in (e_f, e_r, e_d, e_w):
        for k, (e, tol) in errs.items():
            assert e <= tol, (k, e, tol)


def test_fused_backward_as_one_eight_wave_workgroup_per_cu(dev):
    """RES_HALF 0 against 1: bwd_res_kernel 32 x 32 runs as two four-wave workgroups per CU (256 threads, one register set) from
    32 x CUs tiles on, RES_HALF = 0 keeps the eight-wave form (512 threads, two sets of prefetched tiles) -- a different
    instantiation, asserted.  32 x CUs 64-row tiles + one, and 37 ragged rows: the largest case of this file."""
    cu = _cus()
    P = 64 * (32 * cu + 1) + 37
    head = (P // 64) * 64
    assert head // 64 >= 32 * cu and P >= _lib.options()["PN2_RES_MIN_ROWS"]
    run = _layer_run(dev, "bwd", P, 32, 32, 0, 900, tail_from=head)
    _ab("bwd 32 x 32, %d whole-tile rows alone" % head, lambda: run(head), {}, {"PN2_RES_HALF": 0},
        r"^bwd_res_kernel<1, 1, 0, true, 2, false, 512>$", r"^bwd_res_kernel<1, 1, 0, true, 1, false, 256>$")
    with options(PN2_RES_HALF=0):
        n1, e1 = run()
    print("bwd 32 x 32, RES_HALF=0, P = %d = %d + %d: %s  [%s]" % (P, head, P - head, _fmt(e1), _inst(n1)[:80]))
    assert S._streamed(n1), n1
    for k, (e, tol) in e1.items():
        assert e <= tol, (k, e, tol)


def test_wide_pool_off_makes_the_pooled_forward_refuse(dev):
    """WIDE_POOL = 0: pn2_conv1x1_fwd_pool has no kernel for the wide last layers (196 -> 256 over groups of 128) and must say
    so -- PN2_EUNSUPPORTED, nothing launched, nothing written -- so that the caller runs pn2_conv1x1_fwd + pn2_bn_relu_max
    (tests/test_bn_pool_gpu.py).  The default route on the same operands: split_nt_kernel, Y and the sums against fp64."""
    lib = _lib.load()
    K, N, Kp = 196, 256, 128
    P = S._thr("Wd") + Kp
    c, ref = R.fixed_forward_case(dev, P, K, N, 950, affine=True)
    g = torch.Generator(device=dev).manual_seed(951)
    gamma = torch.randn(N, device=dev, generator=g) * 0.5 + 1.0
    G = P // Kp

    def call():
        Yb = R.guarded(P, c["ldy"], dev)
        ws = torch.full((2 * G * N + 64,), R.SENTINEL, dtype=torch.int32, device=dev)
        stats = torch.zeros(R.STAT_REPLICAS * 2 * N, device=dev, dtype=torch.float64)
        lib.pn2_clear_last_kernel()
        rc = lib.pn2_conv1x1_fwd_pool(c["X"].data_ptr(), c["ldx"], c["aff"].data_ptr(), c["W"].data_ptr(), c["ldw"], c["bias"].data_ptr(), Yb.data_ptr(),
                                      c["ldy"], P, K, N, stats.data_ptr(), Kp, gamma.data_ptr(), ws.data_ptr(), None, S._stream())
        torch.cuda.synchronize()
        return rc, S._last(lib), Yb, ws, stats
    rc, name, Yb, ws, stats = call()
    assert rc == 0 and S._is(name, "split_nt_kernel"), (rc, name)
    assert bool((ws[2 * G * N:] == R.SENTINEL).all()) and not bool((ws[:2 * G * N] == R.SENTINEL).any())
    e = S._check_fwd(dev, Yb, stats, ref, 0, P, K, N, "Y")
    print("fwd_pool %d -> %d over %d, %d rows: Y %.2e  sums %.2e %.2e  [%s]" % ((K, N, Kp, P) + e + (_inst(name)[:60],)))
    assert e[0] <= S._y_tol(K) and e[1] <= 1e-5 and e[2] <= 1e-5, e
    with options(PN2_WIDE_POOL=0):
        rc, name, Yb, ws, stats = call()
    assert rc == _lib.PN2_EUNSUPPORTED and name == "", (rc, name)
    assert bool((Yb.view(torch.int32) == R.SENTINEL).all()) and bool((ws == R.SENTINEL).all()) and not bool(stats.any())


# =============================================================================================== (4) two-phase flush

TWO_PHASE_SHAPES = [(256, 196, 128), (256, 128, 64), (196, 128, 0)]              # (C_out, C_in, Kpool) of the full-tile weight gradients


def _pad32(v):
    return (v + 31) // 32 * 32


def test_two_phase_workspace_query_follows_the_options(dev):
    """pn2_conv1x1_wgrad_workspace_bytes: 0 by default; with WGRAD_TWO_PHASE = 1 greater than 0 for 256 x 196 pooled alone,
    with WGRAD_TWO_PHASE_ALL = 1 as well for the three full-tile shapes and nothing else -- one padded slab per CU -- and 0
    below WIDE_WGRAD_MIN_ROWS, for the wrong pooledness, and with WGRAD_TWO_PHASE_ALL alone."""
    lib, cu = _lib.load(), _cus()
    P = S._thr("G") + 128
    q = lib.pn2_conv1x1_wgrad_workspace_bytes
    every = TWO_PHASE_SHAPES + [(128, 128, 0), (256, 196, 0), (196, 128, 64), (256, 256, 128)]
    assert all(q(P, co, ci, int(Kp > 0)) == 0 for co, ci, Kp in every)
    with options(PN2_WGRAD_TWO_PHASE_ALL=1):
        assert all(q(P, co, ci, int(Kp > 0)) == 0 for co, ci, Kp in every)
    size = lambda co, ci: cu * _pad32(co) * _pad32(ci) * 4
    with options(PN2_WGRAD_TWO_PHASE=1):
        assert [q(P, co, ci, int(Kp > 0)) for co, ci, Kp in every] == [size(256, 196), 0, 0, 0, 0, 0, 0]
        assert q(S._thr("G") - 1, 256, 196, 1) == 0
        with options(PN2_WGRAD_TWO_PHASE_ALL=1):
            assert [q(P, co, ci, int(Kp > 0)) for co, ci, Kp in every] == [size(256, 196), size(256, 128), size(196, 128), 0, 0, 0, 0]
            assert q(S._thr("G") - 1, 196, 128, 0) == 0
        with options(PN2_WIDE_WGRAD=0):
            assert q(P, 256, 196, 1) == 0


@pytest.mark.parametrize("co,ci,Kp", TWO_PHASE_SHAPES)
@pytest.mark.parametrize("split", [1, 0])
def test_two_phase_weight_gradient_flush_through_caller_scratch(dev, co, ci, Kp, split):
    """WGRAD_TWO_PHASE = 1 (256 x 196 pooled) and WGRAD_TWO_PHASE_ALL = 1 (all three full-tile shapes) through
    pn2_conv1x1_wgrad_ws, on split_tn_kernel (SPLIT_WGRAD = 1) and on the fp32 wgrad_full_kernel (SPLIT_WGRAD = 0): the
    workspace has exactly the queried size, sits in front of guard words and starts out as NaNs (its contents are
    irrelevant by include/pn2.h); dW of the atomic flush and of the two-phase flush against fp64 within 3e-6.  The flush is
    picked at run time by the workspace pointer: same instantiation (grid-only note of the ledger)."""
    lib = _lib.load()
    P = S._thr("G") + 128
    c, ref = R.fixed_layer_case(dev, P, co, ci, Kp, 1000 + co + ci)
    g = torch.Generator(device=dev).manual_seed(1001)
    rnd = lambda *s_: torch.randn(*s_, device=dev, generator=g)
    GUARD = 64

    def run():
        nbytes = int(lib.pn2_conv1x1_wgrad_workspace_bytes(P, co, ci, int(Kp > 0)))
        assert nbytes % 4 == 0
        ws = torch.full((nbytes // 4 + GUARD,), R.SENTINEL, dtype=torch.int32, device=dev) if nbytes else None
        dW, dW0 = R.framed(co, ci, ci + 4, rnd)
        rc = lib.pn2_conv1x1_wgrad_ws(*c["dz_args"], c["Y"].data_ptr(), c["ldc"], c["coef"].data_ptr(), c["Yp"].data_ptr(), c["ldp"], c["affp"].data_ptr(),
                                      dW.data_ptr(), ci + 4, None, P, co, ci, None, S._p(ws), S._stream())
        assert rc == 0, rc
        name = S._last(lib)
        torch.cuda.synchronize()
        R.check_frame(dW, dW0, co, ci, "dW")
        if ws is not None:
            assert bool((ws[nbytes // 4:] == R.SENTINEL).all()), "written behind the workspace"
            assert not bool((ws[:nbytes // 4] == R.SENTINEL).all()), "the workspace was not used"
        return name + (" [%d workspace bytes]" % nbytes), {"dW": (R.rel(dW[:co, :ci], dW0[:co, :ci].double() + ref["dW"]), BN_TOL)}
    base = {"PN2_SPLIT_WGRAD": split}
    alt = {"PN2_WGRAD_TWO_PHASE": 1} if (co, ci) == (256, 196) else {"PN2_WGRAD_TWO_PHASE": 1, "PN2_WGRAD_TWO_PHASE_ALL": 1}
    with options(**dict(base, **alt)):
        assert lib.pn2_conv1x1_wgrad_workspace_bytes(P, co, ci, int(Kp > 0)) > 0
    _ab("two-phase wgrad %d x %d, K=%d, %d rows" % (co, ci, Kp, P), run, base, alt, grid_only=True,
        base_expect=r"^split_tn_kernel<" if split else r"^wgrad_full_kernel<")


# =============================================================================================== last: nothing left set

def test_zz_options_read_back_at_their_header_defaults(dev):
    """Every test above restores what it set: the library's options equal the defaults of PN2_OPTION_LIST (or what the
    environment of this process forwarded at load time)."""
    import os
    want = O.header_defaults()
    want.update({k: int(os.environ[k]) for k in want if k in os.environ})
    assert _lib.options() == want
