"""GPU: the shared-MLP kernels (MFMA GEMM + BN + ReLU + max, forward and backward) against a plain
PyTorch fp32 (and fp64) statement of the same op on odd shapes the networks never produce."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from pointnet12_amd import _lib
from pointnet12_amd import pointnet_util as U

from mlp_ref import fixed_layer_case as _fixed_layer_case, rel as _rel

pytestmark = pytest.mark.gpu


def torch_mlp(rows, convs, bns, pool, training, dtype):
    y = rows.to(dtype)
    for conv, bn in zip(convs, bns):
        w = conv.weight.reshape(conv.weight.shape[0], -1).to(dtype)
        y = F.linear(y, w, conv.bias.to(dtype))
        if training:
            mean = y.mean(0)
            var = y.var(0, unbiased=False)
        else:
            mean, var = bn.running_mean.to(dtype), bn.running_var.to(dtype)
        y = F.relu((y - mean) / torch.sqrt(var + bn.eps) * bn.weight.to(dtype) + bn.bias.to(dtype))
    if pool:
        y = y.view(-1, pool, y.shape[1]).max(1)[0]
    return y


@pytest.mark.parametrize("P,pool,chans", [
    (4096, 32, [12, 32, 32, 64]), (1000, 0, [7, 20, 196]), (640, 64, [323, 128, 196, 256]),
    (96, 3, [5, 8]), (2048, 16, [67, 64, 300]), (130, 0, [1539, 256, 32]), (32 * 200, 200, [515, 256, 512, 1024]),
    # benchmark-sized rows: the large-P tile choices (64x128 / 128x96 NT, 128x128 / 128x64 / 64x128 TN), the pooled
    # loaders, the streaming first-layer wgrad -- the MSG sa1 stacks at a quarter of their B=16 row count
    (262144, 128, [9, 64, 96, 128]), (262144, 64, [9, 64, 64, 128]), (131072, 0, [137, 128, 196, 256]),
    # the 32-channel stack of sa1 (SSG and MSG scale 1): 32x32 / 64x32 wgrad tiles whose waves split a stage, pooled K = 32;
    # and a few-row stage on the 64x64 wgrad tiles (P <= 65 536)
    (131072, 32, [9, 32, 32, 64]), (65536, 0, [131, 128, 128]),
    # the weight-resident family (csrc/mlp_res.hip): plain first-layer input (unmasked dX, X as stored), pooled K = 64 with a
    # 64-row tile inside one group, 96-wide blocks (three co / ci blocks: dW tiles split by row halves), a ragged tail
    # (P % 64 = 8), and K = 16 < tile rows (four groups per tile)
    (65536, 0, [128, 128, 64]), (131072, 64, [32, 64, 128]), (40008, 0, [96, 96, 32]), (65536, 16, [64, 96, 128]),
    # the register-stationary family (csrc/mlp_wide.hip): the sa2 stacks of MSG-SemSeg -- forward 128->128 / 128->256 /
    # 128->196 / 196->256, dgrad 256->128 and 256->196 on the max-pool's sparse dZ (groups of 64 and of 128), 196->128 and
    # 128->128 dense -- with a ragged tail of whole groups behind the last full tile
    (131072 + 192, 64, [128, 128, 128, 256]), (131072 + 128, 128, [128, 128, 196, 256]), (65536 + 64, 64, [32, 128, 196, 256]),
    # the few-row family (mlp.hip fewrow_nt_kernel: four waves split K, operands straight from global memory): the sa3 stack
    # (group_all-like pooling over 128 rows), the fp3 / fp2 stacks, pooling groups shorter than a tile (16 rows), an odd
    # number of 32-deep stages per wave (K = 576: 18 stages over four waves)
    (2048, 128, [256, 256, 512, 1024]), (2048, 0, [1536, 256, 256]), (8192, 0, [576, 256, 128]), (4096, 16, [320, 128, 128]),
])
def test_shared_mlp_vs_torch(dev, P, pool, chans):
    _check_shared_mlp(dev, P, pool, chans, "positive")


@pytest.mark.parametrize("P,pool,chans", [
    # one pooled and one dense stack at benchmark-sized row counts (the weight-resident, the register-stationary and the streamed
    # kernels with their pooled / dense backward reductions), one small pooled one on the strict bound
    (65536 + 64, 64, [32, 128, 196, 256]), (131072, 0, [137, 128, 196, 256]), (131072, 32, [9, 32, 32, 64]), (640, 16, [12, 32, 64]),
    # round 6: the pooled last layers that run WITHOUT their pre-BN output (pn2_conv1x1_bwd_cf: 128 x 64, 128 x 96) -- negative
    # gamma takes the recorded minimum, gamma = 0 the recomputed row 0
    (65536, 64, [12, 64, 128]), (131072, 128, [32, 96, 128]),
])
def test_shared_mlp_negative_and_zero_gamma(dev, P, pool, chans):
    """VERDICT r4 weak #2 / ADVICE r4: BatchNorm weights of BOTH signs, every fifth one exactly 0, biases in (-1, 1) -- what a trained
    checkpoint holds.  The backward reductions rebuild x-hat from the pooled OUTPUT where |gamma| >= (1 + |beta|) / 4 and from
    Y otherwise (csrc/scatter.hip, HISTORY.md section 4 item 13), the pooling epilogues record the MINIMUM where gamma < 0: with
    gamma in U(-1.5, 1.5) every branch of both selections is taken by some channel, and all of them are held to the fp64
    evaluation (not to each other)."""
    old = _lib.options()["PN2_POOL_CF"]
    _lib.set_option("PN2_POOL_CF", 2)               # (the 128 x 64 output-free form too: the default, PN2_POOL_CF = 2; set here so that the test says what it tests)
    try:
        _check_shared_mlp(dev, P, pool, chans, "signed")
    finally:
        _lib.set_option("PN2_POOL_CF", old)


def _check_shared_mlp(dev, P, pool, chans, gamma_mode):
    gen = torch.Generator().manual_seed(P + len(chans))
    c_in = chans[0]
    ld = (c_in + 3) & ~3
    rows = torch.zeros(P, ld)
    rows[:, :c_in] = torch.randn(P, c_in, generator=gen) * 2 + 0.5
    convs = nn.ModuleList([nn.Conv2d(a, b, 1) for a, b in zip(chans[:-1], chans[1:])])
    bns = nn.ModuleList([nn.BatchNorm2d(b) for b in chans[1:]])
    for bn in bns:
        if gamma_mode == "signed":
            bn.weight.data.uniform_(-1.5, 1.5, generator=gen)
            bn.weight.data[::5] = 0.0
            bn.bias.data.uniform_(-1.0, 1.0, generator=gen)
        else:
            bn.weight.data.uniform_(0.5, 1.5, generator=gen)
            bn.bias.data.uniform_(-0.5, 0.5, generator=gen)
    convs.to(dev), bns.to(dev)
    x = rows.to(dev).requires_grad_(True)
    out = U.shared_mlp(x, c_in, convs, bns, pool, True)
    gw = torch.randn(out.shape, generator=gen).to(dev)
    (out * gw).sum().backward()
    mine = [x.grad[:, :c_in].clone()] + [p.grad.clone() for p in list(convs.parameters()) + list(bns.parameters())]
    rm = [bn.running_mean.clone() for bn in bns]
    rv = [bn.running_var.clone() for bn in bns]

    x64 = rows[:, :c_in].to(dev).double().requires_grad_(True)
    for p in list(convs.parameters()) + list(bns.parameters()):
        p.grad = None
    c64 = nn.ModuleList([nn.Conv2d(a, b, 1) for a, b in zip(chans[:-1], chans[1:])]).to(dev).double()
    b64 = nn.ModuleList([nn.BatchNorm2d(b) for b in chans[1:]]).to(dev).double()
    c64.load_state_dict({k: v.double() for k, v in convs.state_dict().items()})
    b64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in bns.state_dict().items()})
    ref = torch_mlp(x64, c64, b64, pool, True, torch.float64)
    (ref * gw.double()).sum().backward()
    assert float((out.double() - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))
    theirs = [x64.grad] + [p.grad for p in list(c64.parameters()) + list(b64.parameters())]
    # yardstick: the same op in plain torch fp32 on the GPU, measured against the same fp64 answer
    x32 = rows[:, :c_in].to(dev).requires_grad_(True)
    c32 = nn.ModuleList([nn.Conv2d(a, b, 1) for a, b in zip(chans[:-1], chans[1:])]).to(dev)
    b32 = nn.ModuleList([nn.BatchNorm2d(b) for b in chans[1:]]).to(dev)
    c32.load_state_dict(convs.state_dict())
    b32.load_state_dict(b64.state_dict())
    (torch_mlp(x32, c32, b32, pool, True, torch.float32) * gw).sum().backward()
    plain = [x32.grad] + [p.grad for p in list(c32.parameters()) + list(b32.parameters())]
    names = ["x"] + [n for n, _ in list(convs.named_parameters()) + list(bns.named_parameters())]
    for n, a, b, c in zip(names, mine, theirs, plain):
        if n.endswith("bias") and float(a.abs().max()) == 0:
            continue                                  # conv bias before a training-mode BN: exactly 0 here
        scale = max(float(b.abs().max()), 1e-9)
        err = (a.double() - b).abs().flatten()
        err32 = (c.double() - b).abs().flatten()
        # fp32 and fp64 may disagree on a near-tied argmax or on a ReLU input within an ulp of 0 (a flip re-routes
        # one gradient entry), and deep small-batch BN stacks are ill-conditioned in fp32 altogether: be as close
        # to fp64 as 3e-5 of the tensor's max, or within 4x of what plain torch fp32 manages on the same input.
        k = max(1, int(err.numel() * 0.995))
        q, q32 = float(err.kthvalue(k)[0]), float(err32.kthvalue(k)[0])
        # Benchmark-sized cases make 10^5..10^6 argmax / ReLU decisions: ONE of them falling the other way than in fp64
        # re-routes an O(1) output gradient and moves every weight-gradient entry of that channel by ~1/groups of the
        # tensor's max (measured: 1e-3..8e-3 with a single flipped row, 1e-6 with none -- which of the two a given
        # random initialisation gets is luck, for this kernel as for plain torch fp32).  The forward output above is
        # held to 1e-5; here those cases are held to 2e-2 of max, which any indexing or tiling error exceeds by far.
        # (the 200-neighbour group_all-like case makes 32 768 pooled decisions over long, nearly tied rows: same slack)
        # Round 3: the same happens, rarely, from a couple of thousand rows on (2 of 12 repeated runs tripped on the 40 008- and the
        # 8 192-row cases with ONE tensor at 9e-4 of its max while plain torch fp32 itself sat at 1e-4 one time and 2e-6 the
        # other: the per-channel statistics are summed with fp64 atomics whose order changes from run to run, which is enough
        # to push a pre-activation within an ulp of 0 to the other side).  Only the tiny cases stay on the strict bound.
        flip_slack = 2e-2 * scale if (P >= 2048 or pool >= 100) else 0.0
        assert q <= max(3e-5 * scale, 4 * q32, flip_slack), (n, q / scale, q32 / scale)
        # L2 check on everything but the handful of entries a single argmax / ReLU flip re-routes (one flip among the
        # 262 144 pooled decisions of the benchmark-sized cases moves ||err|| by ~1e-3 ||grad|| on its own)
        keep = max(1, err.numel() - max(8, err.numel() // 10000))
        bulk = err.kthvalue(keep)[0]
        assert float(err[err <= bulk].norm()) <= max((2e-2 if (P >= 2048 or pool >= 100) else 1e-3) * float(b.norm()), 4 * float(err32.norm())), n
    # running statistics: momentum 0.1, unbiased variance
    y = x64.detach()
    for l, (conv, bn) in enumerate(zip(c64, b64)):
        y = F.linear(y, conv.weight.reshape(conv.weight.shape[0], -1), conv.bias)
        assert torch.allclose(rm[l].double(), 0.1 * y.mean(0), rtol=1e-5, atol=1e-6)
        assert torch.allclose(rv[l].double(), 0.9 + 0.1 * y.var(0, unbiased=True), rtol=1e-5, atol=1e-6)
        y = F.relu((y - y.mean(0)) / torch.sqrt(y.var(0, unbiased=False) + bn.eps) * bn.weight + bn.bias)


@pytest.mark.parametrize("P,pool,chans", [(131072 + 128, 128, [128, 128, 196, 256]), (131072, 64, [128, 128, 256]), (131072, 0, [128, 128, 128])])
def test_ring_forward_option_is_bit_equal(dev, P, pool, chans):
    """The LDS-DMA ring forward (csrc/mlp_wide.hip ring_fwd_kernel, option PN2_RING, off by default -- DESIGN.md section 3) computes the
    same fp32 fma chain per output element as the register-staged kernel: pooled outputs and every saved pre-BN activation are
    bit-equal, through pn2_set_option (no environment)."""
    gen = torch.Generator().manual_seed(P)
    c_in = chans[0]
    rows = (torch.randn(P, c_in, generator=gen) * 2 + 0.5).to(dev)
    convs = nn.ModuleList([nn.Conv2d(a, b, 1) for a, b in zip(chans[:-1], chans[1:])]).to(dev)
    bns = nn.ModuleList([nn.BatchNorm2d(b) for b in chans[1:]]).to(dev)
    res = {}
    old = _lib.options()["PN2_RING"]
    try:
        for ring in (0, 1):
            _lib.set_option("PN2_RING", ring)
            for bn in bns:
                bn.reset_running_stats()
            out = U.shared_mlp(rows.clone().requires_grad_(True), c_in, convs, bns, pool, True)
            saved = out.grad_fn.saved_tensors
            L = len(chans) - 1
            res[ring] = [out.detach().clone()] + [y.clone() for y in saved[3:3 + L]] + [bn.running_var.clone() for bn in bns]
    finally:
        _lib.set_option("PN2_RING", old)
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)


def test_eval_mode_with_grad(dev):
    gen = torch.Generator().manual_seed(0)
    convs = nn.ModuleList([nn.Conv2d(8, 16, 1), nn.Conv2d(16, 12, 1)]).to(dev)
    bns = nn.ModuleList([nn.BatchNorm2d(16), nn.BatchNorm2d(12)]).to(dev)
    for bn in bns:
        bn.running_mean.uniform_(-0.3, 0.3)
        bn.running_var.uniform_(0.5, 2.0)
    x = torch.randn(512, 8, generator=gen).to(dev).requires_grad_(True)
    out = U.shared_mlp(x, 8, convs, bns, 8, False)
    ref = torch_mlp(x, convs, bns, 8, False, torch.float32)
    assert float((out - ref).abs().max()) <= 1e-5
    gw = torch.randn(out.shape, generator=gen).to(dev)
    ga = torch.autograd.grad((out * gw).sum(), [x] + list(convs.parameters()), retain_graph=True)
    gb = torch.autograd.grad((ref * gw).sum(), [x] + list(convs.parameters()))
    for a, b in zip(ga, gb):
        assert float((a - b).abs().max()) <= 3e-5 * max(float(b.abs().max()), 1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("P,pool,chans", [(262144, 128, [9, 64, 96, 128]), (262144, 64, [9, 64, 64, 128]), (131072, 32, [9, 32, 32, 64]),
                                          (131072 + 64, 0, [12, 64, 64, 96]), (262144, 0, [128, 128, 128, 64])])
def test_bf16_split_kernels_against_the_fp32_pipe(dev, P, pool, chans):
    """Round 5: the same stack through the fp32-pipe kernels (PN2_SPLIT=0: v_mfma_f32_32x32x2_f32, an fp32 fma chain) and through the
    bf16x3 split kernels (split_nt / split_tn / split_bwd_res: six bf16 MFMA products of exact three-way operand splits) -- outputs,
    every saved pre-BN activation and every gradient agree to rounding (1e-5 of the tensor's largest entry; gradients 5e-5: their
    BatchNorm-backward sums run over up to 262 144 rows; input-gradient rows behind a flipped ReLU decision are counted), and the split path must actually have been taken (its results differ in
    the last bits -- bit-equal tensors would mean the option did nothing)."""
    gen = torch.Generator().manual_seed(P + pool)
    c_in = chans[0]
    rows = torch.zeros(P, (c_in + 3) & ~3)                           # [P, round4(c_in)], zero pad columns
    rows[:, :c_in] = torch.randn(P, c_in, generator=gen) * 2 + 0.5
    rows = rows.to(dev)
    convs = nn.ModuleList([nn.Conv2d(a, b, 1) for a, b in zip(chans[:-1], chans[1:])]).to(dev)
    bns = nn.ModuleList([nn.BatchNorm2d(b) for b in chans[1:]]).to(dev)
    gw = None
    res = {}
    old = {k: _lib.options()[k] for k in ("PN2_SPLIT", "PN2_SPLIT_RES")}
    try:
        for arm, (sp, sr) in {"fp32": (0, 0), "split": (1, 2)}.items():
            _lib.set_option("PN2_SPLIT", sp)
            _lib.set_option("PN2_SPLIT_RES", sr)
            for bn in bns:
                bn.reset_running_stats()
            x = rows.clone().requires_grad_(True)
            out = U.shared_mlp(x, c_in, convs, bns, pool, True)
            L = len(chans) - 1
            # (the bf16-pipe arm runs the 128 x 96 pooled last layer without its pre-BN output: no saved tensor to compare there)
            acts = [y.detach().clone() for y in out.grad_fn.saved_tensors[3:3 + L] if y is not None]
            if gw is None:
                gw = torch.randn(out.shape, generator=gen).to(dev)
            grads = torch.autograd.grad((out * gw).sum(), [x] + list(convs.parameters()) + list(bns.parameters()))
            res[arm] = ([out.detach().clone()] + acts, [t.clone() for t in grads])
    finally:
        for k, v in old.items():
            _lib.set_option(k, v)
    differs = False
    for a, b in zip(res["fp32"][0], res["split"][0]):
        assert float((a - b).abs().max()) <= 1e-5 * max(1.0, float(a.abs().max()))
        differs = differs or not torch.equal(a, b)
    for i, (a, b) in enumerate(zip(res["fp32"][1], res["split"][1])):
        bad = (a - b).abs() > 5e-5 * max(float(a.abs().max()), 1e-6)
        if i == 0:
            # the input gradient, row by row: a pre-activation within rounding of 0 takes the other side of its ReLU in the other
            # arithmetic and that ROW's gradient changes by a whole term (the decision flips test_parity_stages_gpu.py counts) --
            # a handful of rows in 1e5, never a pattern
            assert int(bad.any(dim=1).sum()) <= max(8, P // 10000), int(bad.any(dim=1).sum())
        else:
            # parameter gradients sum over all rows, the first layers' through three BatchNorm backward passes: against fp64 BOTH
            # arithmetics sit at 1e-7 .. 6e-5 of the largest entry in the median on these stacks and up to 1e-3 at the entries a
            # flipped decision re-routes, as plain torch fp32 does (tools/exp/split_vs_fp64.py, profiles/r05_split_vs_fp64.txt;
            # the fp64 yardstick with the decisions forced is test_parity_stages_gpu.py's job) -- two such evaluations agree to:
            scale = max(float(a.abs().max()), 1e-6)
            d = (a - b).abs().flatten()
            q995 = float(d.kthvalue(max(1, int(d.numel() * 0.995)))[0])
            assert float(d.median()) <= 1e-3 * scale and q995 <= 2e-2 * scale, (i, float(d.median()), q995, scale)     # (_check_shared_mlp's flip slack)
        differs = differs or not torch.equal(a, b)
    assert differs, "PN2_SPLIT changed nothing: the bf16-split kernels did not run on this stack"


@pytest.mark.gpu
@pytest.mark.parametrize("R,C,weighted,ignored", [(65536, 13, False, False), (1000, 19, True, True), (7, 5, False, True),
                                                  (300001, 50, True, False)])
def test_nll_loss_matches_aten(dev, R, C, weighted, ignored):
    """pn2_nll_loss_fwd/bwd against F.nll_loss (reference semseg.py:143, pcdseg.py:179) in fp64 on the CPU."""
    from pointnet12_amd.loss import nll_loss
    g = torch.Generator().manual_seed(R + C)
    lp = torch.log_softmax(torch.randn(R, C, generator=g) * 3, dim=-1)
    tgt = torch.randint(0, C, (R,), generator=g)
    if ignored:
        tgt[::3] = -100
    w = (torch.rand(C, generator=g) + 0.5) if weighted else None
    ref_in = lp.double().requires_grad_(True)
    ref = F.nll_loss(ref_in, tgt, weight=None if w is None else w.double())
    ref.backward()
    mine_in = lp.to(dev).requires_grad_(True)
    mine = nll_loss(mine_in, tgt.to(dev), weight=None if w is None else w.to(dev))
    (mine * 1.0).backward()
    assert abs(float(mine) - float(ref)) <= 2e-6 * abs(float(ref))          # fp32 products, fp64 sums
    dref = ref_in.grad.float().numpy()
    assert np.abs(mine_in.grad.cpu().numpy() - dref).max() <= 1e-6 * np.abs(dref).max()
    # twice in a row on one stream: the ticket in the workspace resets itself
    again = nll_loss(lp.to(dev), tgt.to(dev), weight=None if w is None else w.to(dev))
    assert float(again) == float(mine)


@pytest.mark.gpu
def test_nll_loss_all_ignored_is_nan(dev):
    from pointnet12_amd.loss import nll_loss
    lp = torch.log_softmax(torch.randn(64, 4), dim=-1).to(dev)
    assert np.isnan(float(nll_loss(lp, torch.full((64,), -100))))
    assert np.isnan(float(F.nll_loss(lp.cpu(), torch.full((64,), -100))))


@pytest.mark.parametrize("P,ci,co", [(70001, 32, 32), (40000, 32, 64), (9000, 20, 32), (150000, 128, 13), (4096, 196, 196),
                                     (300000, 64, 96)])
def test_plain_conv1x1_bias_and_weight_gradients(dev, P, ci, co):
    """The per-point linear layer without BatchNorm (segmentation-head classifier, model/pointnet2.py:174): here the
    bias gradient is NOT zero, so this is the check of the wgrad kernels' column-sum path -- including the 32x32 / 64x32
    tiles whose waves split a stage, the 64x64 few-row tiles and the 128 + remainder column split."""
    import torch.nn as nn
    from pointnet12_amd import pointnet_util as U
    torch.manual_seed(P + ci)
    conv = nn.Conv1d(ci, co, 1).to(dev)
    x = torch.randn(P, ci, device=dev)
    gw = torch.randn(P, co, device=dev)
    xm = x.clone().requires_grad_(True)
    y = U.conv1x1(xm, conv)
    (y * gw).sum().backward()
    mine = [y.detach(), xm.grad, conv.weight.grad.clone(), conv.bias.grad.clone()]
    W, b = conv.weight.detach().double()[:, :, 0], conv.bias.detach().double()
    xd, gd = x.double(), gw.double()
    ref = [xd @ W.t() + b, gd @ W, gd.t() @ xd, gd.sum(0)]
    for name, a, r in zip(("y", "dx", "dW", "db"), mine, ref):
        a = a.double().reshape(r.shape)
        tol = 2e-6 * float(r.abs().max()) * max(1.0, (ci if name in ("y",) else co if name == "dx" else P) ** 0.5 / 8)
        assert float((a - r).abs().max()) <= tol, (name, float((a - r).abs().max()), tol)


@pytest.mark.parametrize("P,pool,chans", [(2048, 128, [256, 256, 512, 1024]), (8192, 0, [576, 256, 128]), (16384, 0, [320, 256, 128]),
                                          (4096, 32, [259, 256, 256, 512]), (65536, 0, [128, 128, 128])])
def test_dgrad_and_wgrad_in_one_launch_equal_the_two_launches(dev, P, pool, chans, monkeypatch):
    """pn2_conv1x1_bwd_pair (round 4): data gradient and weight gradient of a few-row / mid-size layer as ONE call -- one launch
    whose first workgroups run the NT body and the rest the TN body -- against pn2_conv1x1_dgrad followed by
    pn2_conv1x1_wgrad: the same two kernel bodies on the same operands, so the same gradients up to the order of the fp32
    weight-gradient atomics and the fp64 reduction atomics."""
    gen = torch.Generator().manual_seed(P + pool)
    c_in = chans[0]
    ld = (c_in + 3) & ~3
    rows = torch.zeros(P, ld)
    rows[:, :c_in] = torch.randn(P, c_in, generator=gen) * 2 + 0.5
    convs = nn.ModuleList([nn.Conv2d(a, b, 1) for a, b in zip(chans[:-1], chans[1:])])
    bns = nn.ModuleList([nn.BatchNorm2d(b) for b in chans[1:]])
    for bn in bns:
        bn.weight.data.uniform_(0.5, 1.5, generator=gen)
        bn.bias.data.uniform_(-0.5, 0.5, generator=gen)
    convs.to(dev), bns.to(dev)
    res = {}
    # (round 5: from 65 536 rows on the 128 x 128 pair runs in the fused bf16-split kernel by default -- this test is about the
    # pair entry point, so that shape is sent back to it for the duration)
    old = _lib.options()["PN2_SPLIT_RES_MIN_TILES_128"]
    _lib.set_option("PN2_SPLIT_RES_MIN_TILES_128", 4096)
    try:
        _run_pair_arms(dev, monkeypatch, rows, c_in, convs, bns, pool, res)
    finally:
        _lib.set_option("PN2_SPLIT_RES_MIN_TILES_128", old)
    _check_pair_arms(P, res)


def _run_pair_arms(dev, monkeypatch, rows, c_in, convs, bns, pool, res):
    for flag in (True, False):
        monkeypatch.setattr(U, "BWD_PAIR", flag)
        monkeypatch.setattr(U, "_PAIR_RUNS_SPLIT", set())       # (shapes the pair entry point was seen to run as two launches: forgotten here)
        for p in list(convs.parameters()) + list(bns.parameters()):
            p.grad = None
        for bn in bns:
            bn.reset_running_stats()
        x = rows.to(dev).requires_grad_(True)
        with _lib.call_profile() as calls:
            out = U.shared_mlp(x, c_in, convs, bns, pool, True)
            gw = torch.randn(out.shape, generator=torch.Generator().manual_seed(1)).to(dev)
            (out * gw).sum().backward()
            torch.cuda.synchronize()
            names = [c[0] for c in calls]
        res[flag] = (out.detach().clone(), x.grad.clone(), [p.grad.clone() for p in list(convs.parameters()) + list(bns.parameters())], names)


def _check_pair_arms(P, res):
    # (a call that the library ran as two launches is booked as "pn2_conv1x1_bwd_pair_split" by the call profile)
    assert any(n.startswith("pn2_conv1x1_bwd_pair") for n in res[True][3]) and not any(n.startswith("pn2_conv1x1_bwd_pair") for n in res[False][3])
    if P in (8192, 16384, 65536):
        assert "pn2_conv1x1_bwd_pair" in res[True][3]              # these shapes reach the leaf that has a pair instantiation
    assert res[False][3].count("pn2_conv1x1_wgrad") > res[True][3].count("pn2_conv1x1_wgrad")
    assert float((res[True][0] - res[False][0]).abs().max()) <= 1e-6 * max(1.0, float(res[False][0].abs().max()))
    # two separate runs: the statistics atomics land in another order, so a ReLU / arg-max decision within one rounding of its
    # threshold may fall the other way (a rank-one change of the gradients below it): rows of the input gradient beyond 2e-5
    # of its scale are counted, every tensor is held to 1e-2 in L2 (agreement is ~1e-6 when nothing flips)
    xa, xb = res[True][1], res[False][1]
    assert int(((xa - xb).abs().amax(dim=1) > 2e-5 * float(xb.abs().max())).sum()) <= 8
    for a, b in zip([xa] + res[True][2], [xb] + res[False][2]):
        if float(b.abs().max()) == 0.0:
            assert float(a.abs().max()) == 0.0
            continue
        assert float((a - b).norm()) <= 1e-2 * float(b.norm()), float((a - b).norm()) / float(b.norm())


@pytest.mark.parametrize("P,pool,chans", [(65536, 16, [64, 96, 128]), (65536, 32, [32, 32, 64]), (131072, 64, [32, 64, 128]),
                                          (65536, 128, [64, 64, 96]), (32768 + 64, 64, [32, 64, 64]),
                                          # round 4: the register-stationary forward records the extrema too (sa2 of MSG-SemSeg:
                                          # 128 -> 256 on groups of 64, 196 -> 256 on groups of 128)
                                          (131072, 64, [64, 128, 256]), (131072, 128, [64, 196, 256]), (65536, 128, [64, 128, 256])])
def test_pool_in_gemm_epilogue_equals_the_pooling_pass(dev, P, pool, chans):
    """pn2_conv1x1_fwd_pool + pn2_bn_pool_select (extrema of y recorded by the weight-resident GEMM's epilogue, BN + ReLU applied to
    the maximum where the folded scale is >= 0 and to the minimum where it is negative) against pn2_bn_relu_max over Y: the
    pooled output must be BIT-equal (monotonicity), the argmax equal wherever it is unique -- with negative and zero BatchNorm
    weights, and groups padded by repeating their first row (the ball query's padding: equal rows, first one wins)."""
    gen = torch.Generator().manual_seed(P + pool)
    c_in = chans[0]
    rows = torch.randn(P, c_in, generator=gen) * 2 + 0.5
    rows = rows.view(P // pool, pool, c_in)
    rows[::3, pool // 2:] = rows[::3, :1]                       # every third group: second half = copies of its first row
    rows[1::7, 1:] = rows[1::7, :1]                             # some groups: one distinct row only
    rows = rows.reshape(P, c_in).contiguous()
    convs = nn.ModuleList([nn.Conv2d(a, b, 1) for a, b in zip(chans[:-1], chans[1:])])
    bns = nn.ModuleList([nn.BatchNorm2d(b) for b in chans[1:]])
    for bn in bns:
        bn.weight.data.uniform_(-1.5, 1.5, generator=gen)       # half of the channels: negative scale -> the minimum is pooled
        bn.weight.data[::5] = 0.0                               # scale 0: constant output
        bn.bias.data.uniform_(-0.5, 0.5, generator=gen)
    convs.to(dev), bns.to(dev)
    res = {}
    # Bit equality of the two routes needs ONE arithmetic behind both: the narrow last layers have a pooled form on the bf16-split
    # kernel for groups of 64 / 128 only (csrc/mlp_wide.hip, option PN2_SPLIT_NARROW), their plain form stays on the fp32 weight-
    # resident kernel -- equally accurate, different last bits.  The option is pinned off here; the wide shapes below have both
    # forms on the split kernel and are compared with it on.
    narrow_was = _lib.options()["PN2_SPLIT_NARROW"]
    _lib.set_option("PN2_SPLIT_NARROW", 0)
    for flag in (True, False):
        U.POOL_IN_EPILOGUE = flag
        try:
            for p in list(convs.parameters()) + list(bns.parameters()):
                p.grad = None
            for bn in bns:
                bn.reset_running_stats()
            x = rows.to(dev).requires_grad_(True)
            with _lib.call_profile() as calls:
                out = U.shared_mlp(x, c_in, convs, bns, pool, True)
            gw = torch.randn(out.shape, generator=torch.Generator().manual_seed(1)).to(dev)
            (out * gw).sum().backward()
            res[flag] = (out.detach().clone(), x.grad.clone(), [p.grad.clone() for p in convs.parameters()],
                         [c[0] for c in calls])
        finally:
            U.POOL_IN_EPILOGUE = True
            if flag is False:
                _lib.set_option("PN2_SPLIT_NARROW", narrow_was)
    _lib.set_option("PN2_SPLIT_NARROW", narrow_was)
    names_on, names_off = res[True][3], res[False][3]
    assert "pn2_conv1x1_fwd_pool" in names_on and "pn2_bn_pool_select" in names_on and "pn2_bn_relu_max" not in names_on
    assert "pn2_bn_relu_max" in names_off and "pn2_conv1x1_fwd_pool" not in names_off
    assert torch.equal(res[True][0], res[False][0])             # bit-equal pooled output
    # gradients: identical routing except between rows with EQUAL post-BN value (clamped to 0 by the ReLU -- no gradient --
    # or collapsed by rounding).  The two runs are separate launches: the fp64 statistics atomics land in another order, the
    # affine blocks differ in their last bit, and at 131 072+ rows a pair of rows that ties in one run need not tie in the other
    # (seen in round 4, one run in twelve: one re-routed entry = a rank-one change of every weight gradient below it, 3e-3 of
    # its largest entry at 65 536 rows).  So: the input gradient within 1e-4 of its scale on all but a handful of ROWS, and
    # every tensor within 1e-2 in L2.
    xa, xb = res[True][1], res[False][1]
    rows_beyond = int(((xa - xb).abs().amax(dim=1) > 1e-4 * float(xb.abs().max())).sum())
    assert rows_beyond <= 8, rows_beyond
    for a, b in zip([xa] + res[True][2], [xb] + res[False][2]):
        assert float((a - b).norm()) <= 1e-2 * float(b.norm()), float((a - b).norm()) / float(b.norm())


@pytest.mark.parametrize("P,pool,chans", [(262144, 64, [9, 64, 64, 128]), (131072, 32, [9, 32, 32, 64]), (65536, 16, [3, 32, 64]),
                                          (40001, 0, [15, 64, 32]), (8192, 0, [12, 96]), (100000, 0, [6, 128, 64]), (1000, 0, [9, 16]),
                                          (5003, 0, [7, 48]), (5000, 0, [5, 80, 32]), (70, 0, [4, 112])])
def test_first_layer_weight_gradient_closed_form(dev, P, pool, chans, monkeypatch):
    """Round 4 (ABI 9, pn2_conv1x1_wgrad_cf): where the input of a shared MLP needs no gradient, its first
    layer's weight gradient is formed from dZ and the input rows alone -- the BatchNorm-backward terms of dY in closed form from
    the rows' first and second moments -- instead of reading Y as well.  Same layer, same seeds: the closed form against the
    general kernel (PN2_WGRAD_CF = 0) and both against an fp64 statement of the op; every other gradient must not move at all
    beyond the atomics' run-to-run order."""
    gen = torch.Generator().manual_seed(P + chans[0])
    c_in = chans[0]
    ld = (c_in + 3) & ~3
    rows = torch.zeros(P, ld)
    rows[:, :c_in] = torch.randn(P, c_in, generator=gen) * torch.linspace(0.3, 2.0, c_in) + torch.linspace(-1.0, 3.0, c_in)   # non-zero means
    convs = nn.ModuleList([nn.Conv2d(a, b, 1) for a, b in zip(chans[:-1], chans[1:])]).to(dev)
    bns = nn.ModuleList([nn.BatchNorm2d(b) for b in chans[1:]]).to(dev)
    for bn in bns:
        bn.weight.data.uniform_(0.5, 1.5)
        bn.bias.data.uniform_(-0.5, 0.5)
    x = rows.to(dev)
    gw = None
    got = {}
    for cf in (True, False):
        monkeypatch.setattr(U, "WGRAD_CF", cf)
        for p in list(convs.parameters()) + list(bns.parameters()):
            p.grad = None
        for bn in bns:
            bn.reset_running_stats()
        calls = []
        lib = _lib.load()
        orig = lib.pn2_conv1x1_wgrad_cf
        monkeypatch.setattr(lib, "pn2_conv1x1_wgrad_cf", lambda *a: (calls.append(1), orig(*a))[1])
        out = U.shared_mlp(x, c_in, convs, bns, pool, True)
        if gw is None:
            gw = torch.randn(out.shape, generator=gen).to(dev)
        (out * gw).sum().backward()
        monkeypatch.setattr(lib, "pn2_conv1x1_wgrad_cf", orig)
        assert len(calls) == (1 if cf else 0)
        got[cf] = [p.grad.clone() for p in list(convs.parameters()) + list(bns.parameters())]
    x64 = rows[:, :c_in].to(dev).double()
    c64 = nn.ModuleList([nn.Conv2d(a, b, 1) for a, b in zip(chans[:-1], chans[1:])]).to(dev).double()
    b64 = nn.ModuleList([nn.BatchNorm2d(b) for b in chans[1:]]).to(dev).double()
    c64.load_state_dict({k: v.double() for k, v in convs.state_dict().items()})
    b64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in bns.state_dict().items()})
    (torch_mlp(x64, c64, b64, pool, True, torch.float64) * gw.double()).sum().backward()
    ref = c64[0].weight.grad.reshape(chans[1], c_in)
    a, b = got[True][0].reshape(chans[1], c_in).double(), got[False][0].reshape(chans[1], c_in).double()
    scale = float(ref.abs().max())
    ea, eb = float((a - ref).abs().max()) / scale, float((b - ref).abs().max()) / scale
    print("first-layer dW: closed form %.2e, general kernel %.2e of max |dW| from fp64" % (ea, eb))
    # the closed form takes fewer roundings (no per-row fp32 dY): it must be at least as close to fp64 as the general kernel, up to
    # the decision flips both share (same dZ) -- and never further than 3e-5 of the tensor's max beyond it
    assert ea <= eb + 3e-5
    assert float((a - b).abs().max()) / scale <= max(3e-5, 2 * eb)
    names = [n for n, _ in list(convs.named_parameters()) + list(bns.named_parameters())]
    for n, u, v in zip(names[1:], got[True][1:], got[False][1:]):
        s_ = max(float(v.abs().max()), 1e-9)
        assert float((u - v).abs().max()) <= 2e-5 * s_, n                # nothing else reads the changed pass's output


@pytest.mark.gpu
@pytest.mark.parametrize("P,co,ci,Kp", [(65536, 128, 96, 128), (65536, 128, 64, 64), (32768 + 4096, 128, 64, 32), (131072, 128, 96, 64)])
def test_pooled_last_layer_backward_from_its_input_vs_fp64(dev, P, co, ci, Kp):
    """Round 6: pn2_conv1x1_bwd_cf -- the backward of a pooled last layer WITHOUT its pre-BN output (dX = [D | X] W2 + h masked,
    dW from D^T X, the Gram matrix X^T X and the column sums) -- kernel against an fp64 statement of
    dY = c0 dZ + q1 (y - mean) + q0, dX = (dY W) o mask, dW += dY^T X, on fixed inputs with NO decision in the path that rounding
    could flip (the mask is that of the given prev_Y on both sides).  Bounds ~1e-6 of each tensor's largest entry."""
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    old_opt = _lib.options()["PN2_POOL_CF"]
    _lib.set_option("PN2_POOL_CF", 2)
    try:
        _pooled_cf_case(dev, lib, st, P, co, ci, Kp)
    finally:
        _lib.set_option("PN2_POOL_CF", old_opt)


def _pooled_cf_case(dev, lib, st, P, co, ci, Kp):
    assert lib.pn2_conv1x1_bwd_cf_supported(P, co, ci, Kp) == 1
    g = torch.Generator(device=dev).manual_seed(P + ci + Kp)
    rnd = lambda *s_: torch.randn(*s_, device=dev, generator=g)
    G = P // Kp
    Yp = rnd(P, ci) * 1.5 + 0.3
    affp = torch.zeros(4 * ci, device=dev)
    affp[:ci] = rnd(ci) * 0.2                                  # mean
    affp[ci:2 * ci] = (rnd(ci) * 0.5).abs() + 0.3               # scale
    affp[ci:2 * ci][::7] *= -1.0                                # (both signs)
    affp[2 * ci:3 * ci] = rnd(ci) * 0.3                         # beta
    affp[3 * ci:] = (rnd(ci) * 0.2).abs() + 0.8                 # invstd
    W, bias = rnd(co, ci) * 0.2, rnd(co) * 0.1
    coef = torch.zeros(4 * co, device=dev)
    coef[:co] = rnd(co) * 0.5 + 1.0                             # c0
    coef[co:2 * co] = rnd(co) * 1e-3                            # q1
    coef[2 * co:3 * co] = rnd(co) * 1e-3                        # q0
    coef[3 * co:] = rnd(co) * 0.3                               # mean
    dzp = rnd(G, co)
    dzp[rnd(G, co) > 0.5] = 0.0                                 # (outputs that were <= 0 carry nothing)
    arg = torch.randint(0, Kp, (G, co), device=dev, dtype=torch.int32, generator=g)
    dX = torch.empty(P, ci, device=dev)
    red = torch.zeros(8 * 2 * ci, device=dev, dtype=torch.float64)
    dW0 = rnd(co, ci)
    dW = dW0.clone()
    scratch = torch.empty(int(lib.pn2_conv1x1_bwd_cf_scratch_bytes(co, ci)), device=dev, dtype=torch.uint8)
    rc = lib.pn2_conv1x1_bwd_cf(dzp.data_ptr(), co, arg.data_ptr(), Kp, coef.data_ptr(), W.data_ptr(), ci, bias.data_ptr(), Yp.data_ptr(), ci,
                                affp.data_ptr(), dX.data_ptr(), ci, red.data_ptr(), dW.data_ptr(), ci, P, co, ci, None, scratch.data_ptr(), st)
    assert rc == 0
    torch.cuda.synchronize()
    # fp64 statement (the kernels' own mask expression: fma(y - mean, scale, beta) > 0, exact in fp64 on the fp32-rounded difference)
    mean, scale, beta, invstd = (affp[i * ci:(i + 1) * ci] for i in range(4))
    z = (Yp - mean).double() * scale.double() + beta.double()
    X = torch.clamp(z, min=0).float().double()                 # the fp32 activation the kernels stage: max(fma(y - mean, scale, beta), 0)
    mask = z > 0
    D = torch.zeros(G, Kp, co, device=dev, dtype=torch.float64)
    D.scatter_(1, arg.long().unsqueeze(1), dzp.double().unsqueeze(1))
    D = D.view(P, co)
    c0, q1, q0, mu = (coef[i * co:(i + 1) * co].double() for i in range(4))
    Yl = X @ W.double().t() + bias.double()
    dY = c0 * D + q1 * (Yl - mu) + q0
    dX_ref = (dY @ W.double()) * mask
    dW_ref = dW0.double() + dY.t() @ X
    xhat = (Yp - mean).double() * invstd.double()
    r0, r1 = dX_ref.sum(0), (dX_ref * xhat).sum(0)
    redsum = red.view(8, 2, ci).sum(0)

    def rel(a, b):
        return float((a.double() - b).abs().max()) / max(float(b.abs().max()), 1e-30)
    e_dx, e_dw = rel(dX, dX_ref), rel(dW - dW0, dW_ref - dW0.double())
    e_r0, e_r1 = rel(redsum[0], r0), rel(redsum[1], r1)
    print("bwd_cf (%d, %d x %d, K=%d): dX %.2e  dW %.2e  red %.2e %.2e" % (P, co, ci, Kp, e_dx, e_dw, e_r0, e_r1))
    assert e_dx <= 3e-6 and e_dw <= 3e-6 and e_r0 <= 3e-6 and e_r1 <= 3e-6
    # run-to-run identical weight gradient (slabs summed in a fixed order)
    dW2 = dW0.clone()
    red.zero_()
    lib.pn2_conv1x1_bwd_cf(dzp.data_ptr(), co, arg.data_ptr(), Kp, coef.data_ptr(), W.data_ptr(), ci, bias.data_ptr(), Yp.data_ptr(), ci,
                           affp.data_ptr(), dX.data_ptr(), ci, red.data_ptr(), dW2.data_ptr(), ci, P, co, ci, None, scratch.data_ptr(), st)
    torch.cuda.synchronize()
    assert torch.equal(dW, dW2)


@pytest.mark.gpu
@pytest.mark.parametrize("P,co,ci,Kp", [
    # split_bwd_res_kernel (fused data + weight gradient, bf16 pipe): every instantiation of dispatch_bwd_res, dense and pooled
    (131072, 64, 64, 0), (131072, 96, 64, 0), (131072, 128, 128, 0), (131072, 128, 64, 64), (131072, 128, 64, 32), (131072, 128, 96, 128),
    # the fp32-pipe forms that stay (32 x 32, 64 x 32 pooled over 32)
    (131072, 32, 32, 0), (131072, 64, 32, 32)])
def test_fused_backward_kernel_vs_fp64_on_fixed_operands(dev, P, co, ci, Kp):
    """pn2_conv1x1_bwd at kernel level against an fp64 matmul on fixed dZ, Y and X -- no ReLU / arg-max decision that
    rounding could move -- for every shape of the fused kernels, ~1e-6 of each tensor's largest entry (a dropped hi x lo or
    mid x mid term of the split products is 1.5e-5)."""
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    old = _lib.options()["PN2_POOL_CF"]
    _lib.set_option("PN2_POOL_CF", 0)
    try:
        assert lib.pn2_bwd_res_supported(P, co, ci, Kp, 1) == 1
        c, ref = _fixed_layer_case(dev, P, co, ci, Kp, P + co + ci + Kp)
        dX = torch.empty(P, c["ldp"], device=dev)
        red = torch.zeros(8 * 2 * ci, device=dev, dtype=torch.float64)
        dW = torch.zeros(co, ci, device=dev)
        rc = lib.pn2_conv1x1_bwd(*c["dz_args"], c["Y"].data_ptr(), c["ldc"], c["coef"].data_ptr(), c["W"].data_ptr(), ci, c["Yp"].data_ptr(), c["ldp"],
                                 c["affp"].data_ptr(), dX.data_ptr(), c["ldp"], red.data_ptr(), dW.data_ptr(), ci, P, co, ci, None, st)
        assert rc == 0
        torch.cuda.synchronize()
    finally:
        _lib.set_option("PN2_POOL_CF", old)
    redsum = red.view(8, 2, ci).sum(0)
    errs = (_rel(dX[:, :ci], ref["dX"]), _rel(dW, ref["dW"]), _rel(redsum[0], ref["r0"]), _rel(redsum[1], ref["r1"]))
    print("bwd (%d, %d x %d, K=%d): dX %.2e  dW %.2e  red %.2e %.2e" % ((P, co, ci, Kp) + errs))
    assert max(errs) <= 3e-6, errs


@pytest.mark.gpu
@pytest.mark.parametrize("P,co,ci,Kp", [
    # split_tn_kernel (full-tile weight gradients) and split_nt_kernel's data gradients: the sa2 stacks of MSG-SemSeg
    (131072, 256, 196, 128), (131072, 256, 128, 64), (131072, 196, 128, 0), (131072, 128, 128, 0), (262144, 256, 196, 128)])
def test_wide_dgrad_and_wgrad_kernels_vs_fp64_on_fixed_operands(dev, P, co, ci, Kp):
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    c, ref = _fixed_layer_case(dev, P, co, ci, Kp, P + co + ci + Kp + 1)
    dX = torch.empty(P, c["ldp"], device=dev)
    red = torch.zeros(8 * 2 * ci, device=dev, dtype=torch.float64)
    dW = torch.zeros(co, ci, device=dev)
    rc = lib.pn2_conv1x1_dgrad(*c["dz_args"], c["Y"].data_ptr(), c["ldc"], c["coef"].data_ptr(), c["W"].data_ptr(), ci, c["Yp"].data_ptr(), c["ldp"],
                               c["affp"].data_ptr(), dX.data_ptr(), c["ldp"], red.data_ptr(), P, co, ci, None, st)
    assert rc == 0
    rc = lib.pn2_conv1x1_wgrad(*c["dz_args"], c["Y"].data_ptr(), c["ldc"], c["coef"].data_ptr(), c["Yp"].data_ptr(), c["ldp"], c["affp"].data_ptr(),
                               dW.data_ptr(), ci, None, P, co, ci, None, st)
    assert rc == 0
    torch.cuda.synchronize()
    redsum = red.view(8, 2, ci).sum(0)
    errs = (_rel(dX[:, :ci], ref["dX"]), _rel(dW, ref["dW"]), _rel(redsum[0], ref["r0"]), _rel(redsum[1], ref["r1"]))
    print("dgrad + wgrad (%d, %d x %d, K=%d): dX %.2e  dW %.2e  red %.2e %.2e" % ((P, co, ci, Kp) + errs))
    assert max(errs) <= 3e-6, errs


@pytest.mark.gpu
@pytest.mark.parametrize("log2P", [17, 19, 20, 22])
def test_batchnorm_backward_sums_of_the_split_kernels_do_not_drift_with_the_row_count(dev, log2P):
    """the hidden layers' BatchNorm gamma / beta gradients are sums of the masked dX over all rows; on the split
    path a coherent component of the products' error survived that sum (5e-7 .. 2e-6 against 1e-7 on the fp32 pipe).  Round 6 found
    the cause -- v_mfma_f32_32x32x16_bf16 accumulates with a one-sided error, -1.4e-8 of the magnitude whatever the sign
    (tools/exp/split_bias_probe.py), which grows like P in a sum that grows like sqrt(P): 1.4e-6 at 2^17 rows, 5.2e-6 at 2^22 --
    and removed it: odd chunks / tiles are computed negated (csrc/mlp_res.hip, SIGN ALTERNATION).  Pinned here as a function of the
    row count: the two reductions of split_bwd_res_kernel (96 x 64, the 1 M-row layer of sa1) against fp64 on fixed operands stay
    within 1e-6 of their largest entry from 2^17 to 2^22 rows (measured 6e-8 .. 6e-7; cfg5 runs 8 M rows).  The weight gradient's
    accumulators run over all chunks of a workgroup with one sign (dW = (-dY)^T (-X)): its error still grows with the rows (1.6e-6
    at 2^20 on either pipe, 5e-6 at 2^22 on the split pipe against 1.1e-6) and is held to 1e-5."""
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    P, co, ci = 1 << log2P, 96, 64
    c, ref = _fixed_layer_case(dev, P, co, ci, 0, 77 + log2P)
    dX = torch.empty(P, c["ldp"], device=dev)
    red = torch.zeros(8 * 2 * ci, device=dev, dtype=torch.float64)
    dW = torch.zeros(co, ci, device=dev)
    rc = lib.pn2_conv1x1_bwd(*c["dz_args"], c["Y"].data_ptr(), c["ldc"], c["coef"].data_ptr(), c["W"].data_ptr(), ci, c["Yp"].data_ptr(), c["ldp"],
                             c["affp"].data_ptr(), dX.data_ptr(), c["ldp"], red.data_ptr(), dW.data_ptr(), ci, P, co, ci, None, st)
    assert rc == 0
    torch.cuda.synchronize()
    redsum = red.view(8, 2, ci).sum(0)
    # the sums grow like sqrt(P) (random signs) while a coherent error would grow like P: relative to the sum's largest entry
    e0, e1, ew = _rel(redsum[0], ref["r0"]), _rel(redsum[1], ref["r1"]), _rel(dW, ref["dW"])
    print("2^%d rows: sum dX %.2e  sum dX xhat %.2e  dW %.2e" % (log2P, e0, e1, ew))
    assert e0 <= 1e-6 and e1 <= 1e-6 and ew <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("P,co,ci", [(65536, 96, 64), (65536, 64, 64), (131072 + 64, 96, 64)])
def test_fused_backward_with_the_first_layers_sums_vs_fp64(dev, P, co, ci):
    """Round 6: pn2_conv1x1_bwd_first -- the second layer's fused backward forms sum_p dZ1[p, c] x0[p, j] from its dX tiles (dZ1 is
    never written) and pn2_conv1x1_wgrad_cf (dZ == NULL) finishes the FIRST layer's weight gradient from the input's moments -- against
    fp64 on fixed operands: this layer's dW and reductions as in the plain fused backward, the first layer's dW as
    c0 dZ1^T x0 + q1 (W0 S + (b0 - mean0) s^T) + q0 s^T with S, s the input's moments."""
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    old_opt = _lib.options()["PN2_FUSE_FIRST"]
    _lib.set_option("PN2_FUSE_FIRST", 1)               # (the default since the end of round 6; set here so that the test says what it tests)
    try:
        _bwd_first_case(dev, lib, st, P, co, ci)
    finally:
        _lib.set_option("PN2_FUSE_FIRST", old_opt)


def _bwd_first_case(dev, lib, st, P, co, ci):
    assert lib.pn2_conv1x1_bwd_first_supported(P, co, ci, 12) == 1
    c, ref = _fixed_layer_case(dev, P, co, ci, 0, 3 * P + co)
    g = torch.Generator(device=dev).manual_seed(P + 7)
    rnd = lambda *s_: torch.randn(*s_, device=dev, generator=g)
    X0 = rnd(P, 12)
    W0, b0 = rnd(ci, 12) * 0.3, rnd(ci) * 0.1
    coef0 = torch.zeros(4 * ci, device=dev)
    coef0[:ci] = rnd(ci) * 0.5 + 1.0
    coef0[ci:2 * ci] = rnd(ci) * 1e-3
    coef0[2 * ci:3 * ci] = rnd(ci) * 1e-3
    coef0[3 * ci:] = rnd(ci) * 0.3
    red = torch.zeros(8 * 2 * ci, device=dev, dtype=torch.float64)
    dW = torch.zeros(co, ci, device=dev)
    scratch = torch.zeros(int(lib.pn2_conv1x1_wgrad_cf_scratch_bytes()), device=dev, dtype=torch.uint8)
    rc = lib.pn2_conv1x1_bwd_first(*c["dz_args"][:2], c["Y"].data_ptr(), c["ldc"], c["coef"].data_ptr(), c["W"].data_ptr(), ci, c["Yp"].data_ptr(),
                                   c["ldp"], c["affp"].data_ptr(), red.data_ptr(), dW.data_ptr(), ci, X0.data_ptr(), 12, 12, scratch.data_ptr(),
                                   P, co, ci, None, st)
    assert rc == 0
    dW0 = torch.zeros(ci, 12, device=dev)
    rc = lib.pn2_conv1x1_wgrad_cf(None, 0, coef0.data_ptr(), X0.data_ptr(), 12, W0.data_ptr(), 12, b0.data_ptr(), scratch.data_ptr(), dW0.data_ptr(), 12,
                                  P, ci, 12, None, st)
    assert rc == 0
    torch.cuda.synchronize()
    redsum = red.view(8, 2, ci).sum(0)
    x0 = X0.double()
    c0, q1, q0, mu = (coef0[i * ci:(i + 1) * ci].double() for i in range(4))
    S, sv = x0.t() @ x0, x0.sum(0)
    dW0_ref = c0[:, None] * (ref["dX"].t() @ x0) + q1[:, None] * (W0.double() @ S + (b0.double() - mu)[:, None] * sv[None, :]) + q0[:, None] * sv[None, :]
    errs = (_rel(dW, ref["dW"]), _rel(redsum[0], ref["r0"]), _rel(redsum[1], ref["r1"]), _rel(dW0, dW0_ref))
    print("bwd_first (%d, %d x %d): dW %.2e  red %.2e %.2e  first layer's dW %.2e" % ((P, co, ci) + errs))
    assert max(errs) <= 3e-6, errs


@pytest.mark.gpu
@pytest.mark.parametrize("P,pool,chans", [(262144, 128, [9, 64, 96, 128]), (131072, 64, [12, 64, 64, 128])])
def test_shared_mlp_with_the_fused_first_layer_option(dev, P, pool, chans):
    """The whole stack through the Python glue with PN2_FUSE_FIRST=1 (pn2_conv1x1_bwd_first + pn2_conv1x1_wgrad_cf without dZ), held
    to fp64 like every other stack.  (The grouped-row first layer is reached through grouped_mlp in the modules; shared_mlp on
    plain rows takes the same backward branch only with a gather context, so this drives sa1 of a small MSG module instead.)"""
    from pointnet12_amd import pointnet_util as U2
    old_opt = _lib.options()["PN2_FUSE_FIRST"]
    res = {}
    B, N, S, K = 4, 4096, P // pool // 4, pool
    gen = torch.Generator().manual_seed(P)
    xyz = torch.rand(B, 3, N, generator=gen) * 2 - 1
    feat = torch.randn(B, chans[0] - 3, N, generator=gen)
    try:
        for opt in (0, 1):
            _lib.set_option("PN2_FUSE_FIRST", opt)
            torch.manual_seed(7)
            sa = U2.PointNetSetAbstraction(S, 0.4, K, chans[0], chans[1:], False).to(dev).train()
            torch.manual_seed(11)
            with _lib.call_profile() as calls:
                new_xyz, out = sa(xyz.to(dev), feat.to(dev))
                gw = torch.randn(out.shape, generator=torch.Generator().manual_seed(3)).to(dev)
                (out * gw).sum().backward()
                torch.cuda.synchronize()
                names = [c_[0] for c_ in calls]
            assert ("pn2_conv1x1_bwd_first" in names) == bool(opt), names        # (the option really switches the path)
            res[opt] = [out.detach().clone()] + [p.grad.clone() for p in sa.parameters()]
    finally:
        _lib.set_option("PN2_FUSE_FIRST", old_opt)
    for a, b in zip(res[0], res[1]):
        scale = max(float(a.abs().max()), 1e-12)
        assert float((a - b).abs().max()) <= 2e-5 * scale, float((a - b).abs().max()) / scale
