"""GPU: every backward route of ``_SharedMLP`` (pointnet_util._bwd_route) THROUGH the autograd glue, held to fp64 with the
device's own ReLU / arg-max decisions forced (tests/mlp_glue_ref.py), at a few thousand rows.

The kernels behind the routes are held to fp64 at the C ABI elsewhere; this file is about the Python that wires their operands
-- which coefficient block, which reductions, which lazy record, the hand-over from layer 1 to layer 0, the padded weight
copies, the pitch of a ``dest`` slice, ``.grad`` as dW under direct accumulation.  Every case

  * starts from the header's option defaults (whatever earlier tests left is put aside for the case) and an empty
    ``_PAIR_RUNS_SPLIT``; reaches its route by that route's own preconditions -- library options through options_ref.options
    (the row thresholds lowered, as tests/test_mlp_cf_seams_gpu.py reaches "a handful of tiles"), module flags through
    monkeypatch -- and asserts by entry-point name (``_lib.call_profile``) that the route was taken;
  * reads the decisions of the forward from the node's saved tensors, evaluates the same function in fp64 and in stock torch
    float32 with those decisions forced, runs the backward and asserts, none of it fitted to a result of these kernels:
      forward              <= 1e-5 max(1, max|ref|)                              (the rule of _check_shared_mlp)
      running statistics   rtol 1e-5, atol 1e-6
      every gradient       max|hip - ref| <= max(5e-5 max|ref|, 4 max|t32 - ref|)   (FORCED_TOL of test_parity_stages_gpu.py; the
                           factor _check_shared_mlp grants over torch fp32); a reference that is exactly zero asks for exact
                           zeros, and so does the bias in front of a training-mode BatchNorm, whose gradient is 0 by algebra
                           (fp64 autograd leaves 1e-17 there);
  * prints its worst ratio to the bound and how many decisions differ from the unforced fp64 evaluation (information only); the
    worst ratio per route is printed when the module's last case has run and goes from there into the README's table.

Not reached, and why:
  * ``pn2_conv1x1_wgrad_ws`` (the two-phase dW flush of _bwd_streamed): pn2_conv1x1_wgrad_workspace_bytes is non-zero for
    256 x 196, 256 x 128 and 196 x 128 only (csrc/mlp_wide.hip, pn2_wide_wgrad_workspace_bytes), whatever PN2_WGRAD_TWO_PHASE /
    PN2_WIDE_WGRAD_MIN_ROWS say: no stack of at most 128 channels has such a layer.  The kernel itself is held to fp64 at
    65 536 rows by test_options_mlp_gpu.py::test_two_phase_weight_gradient_flush_through_caller_scratch.
  * the from-input route with groups of 32: pn2_conv1x1_bwd_cf_supported accepts K = 32, but the forward has an output-free
    form for groups of 64 and 128 only (csrc/mlp_wide.hip, SPLIT_FWD(.., 64) / (.., 128)); with K = 32 _fwd_pooled_last falls
    back to the launch that writes Y, and the layer takes the resident (128 x 64) or the streamed (128 x 96) route.  Those two
    stacks are run below as what they are; from-input runs at K = 64 and K = 128.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import geometry as G
from pointnet12_amd import _lib
from pointnet12_amd import pointnet_util as U

import mlp_glue_ref as R
import options_ref as O

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
LD_WIDE, COL0 = 320, 64              # the concatenated MSG output's pitch; where the slice of a ``dest`` case starts
REPORT = {}


def _report(route, tag, ratio, differing):
    r = REPORT.setdefault(route, {"worst_ratio": 0.0, "cases": 0, "decisions_differing": 0})
    r["worst_ratio"] = max(r["worst_ratio"], ratio)
    r["cases"] += 1
    r["decisions_differing"] += differing


@pytest.fixture(scope="module", autouse=True)
def _route_table():
    """After the module's last case: one line per route (shown with ``-s``), the rows of the README's table."""
    yield
    for route, r in sorted(REPORT.items()):
        print("\nroute %-45s %3d cases, worst error / bound %.3f, %d decisions differ" % (route, r["cases"], r["worst_ratio"], r["decisions_differing"]))


@pytest.fixture(autouse=True)
def _isolated(dev, monkeypatch):
    """Header defaults for every library option and module flag the routes read, and nothing remembered about the pair call."""
    monkeypatch.setattr(U, "_PAIR_RUNS_SPLIT", set())
    for flag, value in (("BWD_PAIR", True), ("WGRAD_CF", True), ("LAZY_BN", True), ("POOL_IN_EPILOGUE", True), ("GATHER_CONV", True),
                        ("DWX_REPLICAS_SCRATCH", True), ("ALIGN_WEIGHT_MIN_ROWS", 32768)):
        monkeypatch.setattr(U, flag, value)
    assert not U._DIRECT_GRADS
    with O.options(**O.header_defaults()):
        monkeypatch.setattr(U, "_PAIR_RUNS_SPLIT", set())           # (set_option clears the set it finds: a fresh one for the case)
        yield


def _modules(dev, weights, bn_params, training):
    convs = nn.ModuleList([nn.Conv2d(w.shape[1], w.shape[0], 1) for w, _ in weights])
    bns = nn.ModuleList([nn.BatchNorm2d(w.shape[0]) for w, _ in weights])
    with torch.no_grad():
        for conv, bn, (w, b), (gamma, beta, rmean, rvar, eps) in zip(convs, bns, weights, bn_params):
            conv.weight.copy_(w.view_as(conv.weight)), conv.bias.copy_(b)
            bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rmean), bn.running_var.copy_(rvar)
            assert bn.eps == eps
    return convs.to(dev), bns.to(dev)


class _Rows:
    """shared_mlp on plain rows [P, round4(C_0)]."""

    def __init__(self, dev, P, pool, chans, seed=0, training=True, rows_grad=True):
        self.dev, self.P, self.pool, self.chans, self.training, self.in_grad = dev, P, pool, chans, training, rows_grad
        self.rows, self.weights, self.bn_params = R.make_case(P, pool, chans, seed + P + len(chans), training)
        self.convs, self.bns = _modules(dev, self.weights, self.bn_params, training)
        self.G = P // pool if pool else P

    def forward(self, dest):
        c = self.chans[0]
        x = torch.zeros(self.P, (c + 3) & ~3)
        x[:, :c] = self.rows
        self.x = x.to(self.dev).requires_grad_(self.in_grad)
        return U.shared_mlp(self.x, c, self.convs, self.bns, self.pool, self.training, dest=dest)

    def input_grad(self):
        return self.x.grad[:, :self.chans[0]]

    def ref_rows(self, dtype):
        leaf = self.rows.to(self.dev, dtype).requires_grad_(self.in_grad)
        return leaf, leaf


class _Grouped:
    """grouped_mlp on un-grouped points [B, N, D] with a ball-query index [B, S, K]: the gather-conv first layer (D <= 9) or the
    factorised one (D >= 32).  The reference builds the grouped rows itself, xyz[idx] - centre in float32 as pn2_group stores it."""

    def __init__(self, dev, xyz, new_xyz, idx, D, chans, xyz_first, seed=0, points_grad=False, with_inv=False):
        B, S, K = idx.shape
        self.dev, self.P, self.pool, self.chans, self.training, self.in_grad = dev, B * S * K, K, chans, True, points_grad
        assert chans[0] == 3 + D
        _, self.weights, self.bn_params = R.make_case(8, K, chans, seed + D + len(chans), True)
        self.convs, self.bns = _modules(dev, self.weights, self.bn_params, True)
        self.points = torch.randn(B, xyz.shape[1], D, generator=torch.Generator().manual_seed(seed + D)) * 1.5 + 0.25
        self.xyz, self.new_xyz, self.idx, self.xyz_first = xyz.to(dev), new_xyz.to(dev), idx.to(dev), xyz_first
        self.inv = U._group_inverse(self.idx, xyz.shape[1], D, len(chans) - 1, True) if with_inv else None
        assert (self.inv is not None) == with_inv
        self.G = B * S

    def forward(self, dest):
        self.x = self.points.to(self.dev).requires_grad_(self.in_grad)
        return U.grouped_mlp(self.xyz, self.x, self.new_xyz, self.idx, self.xyz_first, self.convs, self.bns, True, inv=self.inv, dest=dest)

    def input_grad(self):
        return self.x.grad

    def ref_rows(self, dtype):
        leaf = self.points.to(self.dev, dtype).requires_grad_(self.in_grad)
        B = self.idx.shape[0]
        b = torch.arange(B, device=self.dev)[:, None, None]
        gx = (self.xyz[b, self.idx] - self.new_xyz[:, :, None, :]).to(dtype)
        gp = leaf[b, self.idx]
        return leaf, torch.cat([gx, gp] if self.xyz_first else [gp, gx], -1).reshape(self.P, -1)


def _reference(case, dec, gw, dtype):
    """{name: gradient}, output and ``made`` of the forced function (decisions None: the function as it stands) in ``dtype``."""
    dev = case.dev
    leaf, rows = case.ref_rows(dtype)
    ws = [(w.to(dev, dtype).requires_grad_(True), b.to(dev, dtype).requires_grad_(True)) for w, b in case.weights]
    bs = [(g.to(dev, dtype).requires_grad_(True), be.to(dev, dtype).requires_grad_(True), rm.to(dev, dtype), rv.to(dev, dtype), eps)
          for g, be, rm, rv, eps in case.bn_params]
    out, made = R.forced_mlp(rows, ws, bs, case.pool, case.training, dec, dtype)
    (out * gw.to(dtype)).sum().backward()
    g = {"input": leaf.grad} if case.in_grad else {}
    for l, ((w, b), bn) in enumerate(zip(ws, bs)):
        g["W%d" % l], g["bias%d" % l], g["gamma%d" % l], g["beta%d" % l] = w.grad, b.grad, bn[0].grad, bn[1].grad
    return g, out.detach(), made


def _params(case):
    """{name: parameter} in the names of _reference."""
    p = {}
    for l, (conv, bn) in enumerate(zip(case.convs, case.bns)):
        p["W%d" % l], p["bias%d" % l], p["gamma%d" % l], p["beta%d" % l] = conv.weight, conv.bias, bn.weight, bn.bias
    return p


def _hold(case, route, tag, expect=(), forbid=(), direct=False, dest=False):
    """One forward + backward of ``case`` through the glue, held to the forced references (module docstring) -> the entry points
    it called, in order."""
    dev, pool, training, cl = case.dev, case.pool, case.training, case.chans[-1]
    params = _params(case)
    for q in params.values():
        q.grad = None
    if training:
        for bn in case.bns:
            bn.reset_running_stats()
    stats_before = [(bn.running_mean.clone(), bn.running_var.clone()) for bn in case.bns]
    gw = torch.randn(case.G, cl, generator=torch.Generator().manual_seed(case.P + cl)).to(dev)
    big = torch.full((case.G, LD_WIDE), SENTINEL, device=dev) if dest else None
    with _lib.call_profile() as calls:
        out = case.forward((big, COL0) if dest else None)
        assert tuple(out.shape) == (case.G, cl)
        if dest:
            assert out.data_ptr() == big.data_ptr() + 4 * COL0 and out.stride(0) == LD_WIDE
        node = R.mlp_node(out)
        no_last_y = node.saved_tensors[3 + len(case.chans) - 2] is None
        dec = R.decisions_of(out)
        ref, ref_out, made = _reference(case, dec, gw, torch.float64)
        t32, _, _ = _reference(case, dec, gw, torch.float32)
        _, _, made_plain = _reference(case, None, gw, torch.float64)
        differing = R.decisions_differing(dec, made_plain)
        hip_out = out.detach().clone()
        prefill = {}
        if direct:
            for k, q in params.items():
                prefill[k] = R.prefill_like(torch.zeros_like(ref[k]) if (training and k.startswith("bias")) else ref[k]).float().view_as(q)
                q.grad = prefill[k].clone()
            U.set_direct_grad_accumulation(True)
        try:
            if dest:                                                    # the upstream gradient as the matching slice, pitch 320
                gbig = torch.full((case.G, LD_WIDE), 7.0, device=dev)
                gbig[:, COL0:COL0 + cl] = gw
                torch.autograd.backward([out], [gbig[:, COL0:COL0 + cl]])
            else:
                torch.autograd.backward([out], [gw])
        finally:
            if direct:
                U.set_direct_grad_accumulation(False)
        torch.cuda.synchronize()
        names = [c[0] for c in calls]
    for n in expect:
        assert n in names, (tag, "expected " + n, names)
    for n in forbid:
        assert not any(m.startswith(n) for m in names), (tag, "unexpected " + n, names)
    # ---- forward, the frame of a dest slice, running statistics
    assert float((hip_out.double() - ref_out).abs().max()) <= 1e-5 * max(1.0, float(ref_out.abs().max())), tag
    if dest:
        outside = torch.cat([big[:, :COL0], big[:, COL0 + cl:]], 1)
        assert bool((outside == SENTINEL).all()), (tag, "columns outside the dest slice were written")
        assert torch.equal(big[:, COL0:COL0 + cl], hip_out), (tag, "the dest slice changed in the backward")
    for l, (bn, (m0, v0)) in enumerate(zip(case.bns, stats_before)):
        if training:
            mean, var = made["stats"][l]
            assert torch.allclose(bn.running_mean.double(), 0.9 * m0.double() + 0.1 * mean, rtol=1e-5, atol=1e-6), (tag, l)
            assert torch.allclose(bn.running_var.double(), 0.9 * v0.double() + 0.1 * var, rtol=1e-5, atol=1e-6), (tag, l)
        else:
            assert torch.equal(bn.running_mean, m0) and torch.equal(bn.running_var, v0), (tag, l)
    # ---- gradients
    got = {k: q.grad.reshape(ref[k].shape) for k, q in params.items()}
    if case.in_grad:
        got["input"] = case.input_grad()
    else:
        assert case.x.grad is None
    worst, bad = 0.0, []
    for k, g in got.items():
        if training and k.startswith("bias"):                         # 0 by algebra: nothing is added to what .grad held
            want = prefill[k].reshape(g.shape) if direct else torch.zeros_like(g)
            if not torch.equal(g, want):
                bad.append((k, "not exactly %s" % ("the pre-fill" if direct else "zero")))
            continue
        want = ref[k] + prefill[k].double().reshape(ref[k].shape) if (direct and k in prefill) else ref[k]
        err = float((g.double() - want).abs().max())
        if float(ref[k].abs().max()) == 0.0:
            ratio = 0.0 if err == 0.0 else float("inf")
        else:
            ratio = err / R.grad_bound(ref[k], t32[k])
        worst = max(worst, ratio)
        if not ratio <= 1.0:
            bad.append((k, ratio, err, float(ref[k].abs().max()), float((t32[k].double() - ref[k]).abs().max())))
    print("%s / %s: worst ratio to the bound %.3g, %d decisions differ from plain fp64%s" %
          (route, tag, worst, differing, " (no Y of the last layer)" if no_last_y else ""))
    _report(route, tag, worst, differing)
    assert not bad, (route, tag, bad)
    return names, no_last_y


# ================================================================================================= streamed

@pytest.mark.parametrize("rows_grad", [True, False])
@pytest.mark.parametrize("P,pool,chans", [(1041, 0, [20, 32, 13]), (2064, 16, [9, 32, 64])])
def test_streamed_route(dev, monkeypatch, P, pool, chans, rows_grad):
    monkeypatch.setattr(U, "BWD_PAIR", False)
    names, _ = _hold(_Rows(dev, P, pool, chans, rows_grad=rows_grad), "streamed", "%s rows_grad=%d" % (chans, rows_grad),
                     expect=("pn2_conv1x1_dgrad", "pn2_conv1x1_wgrad"), forbid=("pn2_conv1x1_bwd",))
    assert names.count("pn2_conv1x1_dgrad") == len(chans) - 2 + int(rows_grad)


@pytest.mark.parametrize("cf", [True, False])
def test_streamed_route_with_the_closed_form_first_layer(dev, monkeypatch, cf):
    monkeypatch.setattr(U, "BWD_PAIR", False)
    monkeypatch.setattr(U, "WGRAD_CF", cf)
    _hold(_Rows(dev, 1041, 0, [9, 64, 64], rows_grad=False), "streamed, closed-form first layer", "WGRAD_CF=%d" % cf,
          expect=("pn2_conv1x1_wgrad_cf",) if cf else ("pn2_conv1x1_wgrad",), forbid=("pn2_conv1x1_bwd",) + (() if cf else ("pn2_conv1x1_wgrad_cf",)))


@pytest.mark.parametrize("P,pool,chans,mode", [(1041, 0, [20, 32, 13], "direct"), (1041, 0, [20, 32, 13], "lazy-off"), (2064, 16, [9, 32, 64], "direct"),
                                               (2064, 16, [9, 32, 64], "lazy-off"), (2064, 16, [9, 32, 64], "dest")])
def test_streamed_route_variants(dev, monkeypatch, P, pool, chans, mode):
    monkeypatch.setattr(U, "BWD_PAIR", False)
    if mode == "lazy-off":
        monkeypatch.setattr(U, "LAZY_BN", False)
    names, _ = _hold(_Rows(dev, P, pool, chans, seed=3), "streamed", "%s %s" % (chans, mode), direct=mode == "direct", dest=mode == "dest",
                     expect=("pn2_conv1x1_dgrad", "pn2_conv1x1_wgrad") + (("pn2_bn_bwd_coef", "pn2_bn_finalize") if mode == "lazy-off" else ()),
                     forbid=("pn2_conv1x1_bwd",) + (() if mode == "lazy-off" else ("pn2_bn_bwd_coef", "pn2_bn_finalize")))


def test_eval_mode_with_gradients_on_the_streamed_route(dev):
    """training=False: running statistics away from (0, 1) and untouched by the step, dbias from the weight-gradient kernel."""
    names, _ = _hold(_Rows(dev, 1041, 0, [20, 32, 13], training=False), "streamed, eval mode", "[20, 32, 13]",
                     expect=("pn2_conv1x1_dgrad", "pn2_conv1x1_wgrad"), forbid=("pn2_conv1x1_bwd",))
    _hold(_Rows(dev, 2064, 16, [9, 32, 64], training=False), "streamed, eval mode", "[9, 32, 64] pooled",
          expect=("pn2_conv1x1_dgrad", "pn2_conv1x1_wgrad"), forbid=("pn2_conv1x1_bwd",))


def test_direct_accumulation_in_eval_mode_raises(dev):
    case = _Rows(dev, 1041, 0, [20, 32, 13], training=False)
    out = case.forward(None)
    for q in _params(case).values():
        q.grad = torch.ones_like(q)
    U.set_direct_grad_accumulation(True)
    try:
        with pytest.raises(NotImplementedError):
            out.sum().backward()
    finally:
        U.set_direct_grad_accumulation(False)


# ================================================================================================= pair

@pytest.mark.parametrize("mode", ["plain", "direct"])
def test_pair_route_in_one_launch(dev, mode):
    """The weight-gradient half rides in the data gradient's launch on the 64 x 128 tile only (csrc/mlp.hip, launch_nt).  At
    8192 rows a 128 -> 128 data gradient is 512 few-row tiles, which fewrow_nt_kernel takes, and 128 x 1 x 2 = 256 tiles of
    64 x 64, which the few-row configuration takes on 256 CUs: by default no stack of <= 128 channels and <= 8192 rows reaches
    the pair body (the library answers PN2_OK_SPLIT, the case below this one).  PN2_FEWROW_MAX_TILES_DGRAD = 0 and PN2_NT_CFG = 7
    send the shape to the 64 x 128 tile, where pn2_conv1x1_bwd_pair has its instantiation."""
    with O.options(PN2_SPLIT_RES_MIN_TILES_128=4096, PN2_FEWROW_MAX_TILES_DGRAD=0, PN2_NT_CFG=7):
        _hold(_Rows(dev, 8192, 0, [128, 128, 128]), "pair", "[128, 128, 128] %s" % mode, direct=mode == "direct",
              expect=("pn2_conv1x1_bwd_pair",), forbid=("pn2_conv1x1_dgrad",))


@pytest.mark.parametrize("mode", ["plain", "direct"])
def test_pair_route_answers_split_and_the_next_step_takes_the_streamed_route(dev, mode):
    """64 x 64 has no pair instantiation: the library runs its own two launches and answers PN2_OK_SPLIT; from the second step
    on the same shape goes through _bwd_streamed.  Step 1 and step 2 run different glue: both are held to the reference."""
    case = _Rows(dev, 2050, 0, [20, 64, 64])
    _hold(case, "pair, PN2_OK_SPLIT", "step 1 %s" % mode, direct=mode == "direct", expect=("pn2_conv1x1_bwd_pair_split",), forbid=("pn2_conv1x1_dgrad",))
    assert (2050, 64, 64, False, True) in U._PAIR_RUNS_SPLIT
    names, _ = _hold(case, "pair, PN2_OK_SPLIT", "step 2 %s" % mode, direct=mode == "direct", expect=("pn2_conv1x1_dgrad", "pn2_conv1x1_wgrad"),
                     forbid=("pn2_conv1x1_bwd_pair",))
    assert names.count("pn2_conv1x1_dgrad") == 2 and names.count("pn2_conv1x1_wgrad") == 2
    _lib.set_option("PN2_BWD_PAIR", 1)                                  # (its value: any pn2_set_option forgets the shapes)
    assert not U._PAIR_RUNS_SPLIT
    _hold(case, "pair, PN2_OK_SPLIT", "step 3, after pn2_set_option %s" % mode, direct=mode == "direct", expect=("pn2_conv1x1_bwd_pair_split",))


# ================================================================================================= resident

RES_ROWS = dict(PN2_RES_MIN_ROWS=64)


@pytest.mark.parametrize("chans,mode", [([12, 32, 32], "plain"), ([12, 64, 64], "plain"), ([12, 64, 96], "plain"),
                                        ([12, 64, 64], "direct"), ([12, 64, 96], "lazy-off")])
def test_resident_route_dense_masked_with_a_ragged_tail(dev, monkeypatch, chans, mode):
    if mode == "lazy-off":
        monkeypatch.setattr(U, "LAZY_BN", False)
    with O.options(**RES_ROWS):
        assert _lib.load().pn2_bwd_res_supported(64 * 16 + 17, chans[2], chans[1], 0, 1) == 1
        _hold(_Rows(dev, 64 * 16 + 17, 0, chans), "resident, dense", "%s %s" % (chans, mode), direct=mode == "direct", expect=("pn2_conv1x1_bwd",))


@pytest.mark.parametrize("co,ci,K,mode", [(128, 64, 64, "plain"), (128, 96, 64, "plain"), (64, 32, 32, "plain"), (128, 64, 32, "plain"),
                                          (128, 64, 64, "direct"), (128, 64, 32, "dest"), (128, 96, 64, "lazy-off"), (64, 32, 32, "direct"),
                                          (128, 96, 64, "dest")])
def test_resident_route_pooled(dev, monkeypatch, co, ci, K, mode):
    if mode == "lazy-off":
        monkeypatch.setattr(U, "LAZY_BN", False)
    P = 33 * 64 if K == 64 else 65 * 32                                 # G odd: K = 32 leaves a 32-row half tile
    with O.options(PN2_POOL_CF=0, **RES_ROWS):                          # (POOL_CF = 0: Y is kept)
        assert _lib.load().pn2_bwd_res_supported(P, co, ci, K, 1) == 1
        _, no_y = _hold(_Rows(dev, P, K, [12, ci, co]), "resident, pooled", "%d x %d K=%d %s" % (co, ci, K, mode), direct=mode == "direct",
                        dest=mode == "dest", expect=("pn2_conv1x1_bwd", "pn2_pool_bwd_reduce_ld"), forbid=("pn2_conv1x1_bwd_cf",))
        assert not no_y


# ================================================================================================= from input

@pytest.mark.parametrize("ci,K,mode", [(64, 64, "plain"), (96, 64, "plain"), (96, 128, "plain"), (96, 64, "direct"), (64, 64, "dest"), (96, 128, "dest")])
def test_from_input_route(dev, ci, K, mode):
    P = 34 * K                                                          # (the output-free forward takes whole 128-row units)
    with O.options(PN2_POOL_CF=2, PN2_WIDE_MIN_ROWS=128, **RES_ROWS):
        _, no_y = _hold(_Rows(dev, P, K, [12, ci, 128]), "from input", "128 x %d K=%d %s" % (ci, K, mode), direct=mode == "direct", dest=mode == "dest",
                        expect=("pn2_conv1x1_bwd_cf", "pn2_pool_bwd_reduce_rec"), forbid=("pn2_pool_bwd_reduce_ld",))
        assert no_y, "saved_tensors holds a Y for the last layer"


@pytest.mark.parametrize("ci", [64, 96])
def test_groups_of_32_keep_their_output_and_take_another_route(dev, ci):
    """(module docstring) pn2_conv1x1_bwd_cf_supported says yes, the forward has no output-free form: Y is written."""
    P = 65 * 32
    with O.options(PN2_POOL_CF=2, PN2_WIDE_MIN_ROWS=128, **RES_ROWS):
        assert _lib.load().pn2_conv1x1_bwd_cf_supported(P, 128, ci, 32) == 1
        names, no_y = _hold(_Rows(dev, P, 32, [12, ci, 128]), "resident, pooled" if ci == 64 else "pair", "128 x %d K=32, POOL_CF=2" % ci,
                            expect=("pn2_pool_bwd_reduce_ld",), forbid=("pn2_conv1x1_bwd_cf",))
        assert not no_y
        assert "pn2_conv1x1_bwd" in names if ci == 64 else any(n.startswith("pn2_conv1x1_bwd_pair") for n in names), names


# ================================================================================================= fused first (gather-conv first layer)

def _random_groups(B, N, S, K, seed):
    gen = torch.Generator().manual_seed(seed)
    xyz = torch.rand(B, N, 3, generator=gen) * 2 - 1
    idx = torch.randint(0, N, (B, S, K), generator=gen)
    return xyz, xyz[:, :S].contiguous(), idx


@pytest.mark.parametrize("D,c2,mode", [(D, c2, m) for D in (6, 9) for c2 in (64, 96) for m in ("plain", "points-grad")] +
                         [(9, 96, "direct"), (6, 64, "direct"), (9, 64, "dest")])
def test_fused_first_route(dev, D, c2, mode):
    xyz, new_xyz, idx = _random_groups(2, 256, 33, 32, D + c2)           # B S K = 2112 = 33 x 64 rows
    case = _Grouped(dev, xyz, new_xyz, idx, D, [3 + D, 64, c2, 128], xyz_first=True, points_grad=mode == "points-grad")
    with O.options(PN2_FUSE_FIRST=1, **RES_ROWS):
        if mode == "points-grad":                                       # somebody wants d rows: the stack takes its ordinary routes
            _hold(case, "gather-conv, with a points gradient", "[%d, 64, %d, 128]" % (3 + D, c2), expect=("pn2_group_conv_fwd", "pn2_conv1x1_bwd", "pn2_group_bwd"),
                  forbid=("pn2_conv1x1_bwd_first", "pn2_conv1x1_wgrad_cf"))
        else:
            _hold(case, "fused first", "[%d, 64, %d, 128] %s" % (3 + D, c2, mode), direct=mode == "direct", dest=mode == "dest",
                  expect=("pn2_group_conv_fwd", "pn2_conv1x1_bwd_first", "pn2_conv1x1_wgrad_cf"), forbid=("pn2_group_bwd",))


# ================================================================================================= factorised first layer

_geometry = {}


def _ball_groups():
    """A 512-point cloud twice (B = 2), 64 FPS centres, 16 neighbours within 0.35: oracle.geometry, computed once."""
    if not _geometry:
        rng = np.random.RandomState(5)
        xyz = (rng.rand(2, 512, 3) * 2 - 1).astype(np.float32)
        fps = G.farthest_point_sample(xyz, 64, np.array([3, 100]))
        new = G.index_points(xyz, fps)
        idx = G.query_ball_point(0.35, 16, xyz, new)
        assert idx.max() < 512
        _geometry["g"] = (torch.from_numpy(xyz), torch.from_numpy(np.ascontiguousarray(new, dtype=np.float32)), torch.from_numpy(idx))
    return _geometry["g"]


@pytest.mark.parametrize("feat_grad", [True, False])
@pytest.mark.parametrize("scatter", ["segmented", "segmented, no replica scratch", "atomics"])
@pytest.mark.parametrize("D,xyz_first", [(33, False), (40, True)])
def test_factorised_first_layer(dev, monkeypatch, D, xyz_first, scatter, feat_grad):
    monkeypatch.setattr(U, "DWX_REPLICAS_SCRATCH", scatter == "segmented")
    xyz, new_xyz, idx = _ball_groups()
    case = _Grouped(dev, xyz, new_xyz, idx, D, [3 + D, 64, 64], xyz_first, points_grad=feat_grad, with_inv=scatter != "atomics")
    seg = "pn2_group_affine_bwd_seg"
    names, _ = _hold(case, "factorised first layer", "D=%d %s feat_grad=%d" % (D, scatter, feat_grad),
                     expect=("pn2_group_affine_fwd", "pn2_conv1x1_bwd_pair_split") + ((seg,) if scatter != "atomics" else ("pn2_group_affine_bwd", "pn2_bn_bwd_coef")),
                     forbid=("pn2_group_bwd",) + (("pn2_bn_bwd_coef",) if scatter != "atomics" else (seg,)))
    assert ("pn2_copy_cols" in names) == (D == 33)                      # the zero-padded copy of the feature columns (features first, D % 4 == 1)
    assert names.count("pn2_conv1x1_dgrad") == int(feat_grad)           # (the feature gradient's GEMM; layer 1 went through the pair call)


@pytest.mark.parametrize("D,xyz_first", [(33, False), (40, True)])
def test_factorised_first_layer_under_direct_accumulation(dev, D, xyz_first):
    xyz, new_xyz, idx = _ball_groups()
    case = _Grouped(dev, xyz, new_xyz, idx, D, [3 + D, 64, 64], xyz_first, points_grad=True, with_inv=True)
    _hold(case, "factorised first layer", "D=%d direct" % D, direct=True, expect=("pn2_group_affine_bwd_seg",))
