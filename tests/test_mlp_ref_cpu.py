"""tests/mlp_ref.py against PyTorch's own fp64 BatchNorm and autograd, on the CPU: the reference the GEMM seam tests hold the
kernels to must itself be the operation of model/pointnet_util.py (relu(batch_norm(conv)), training mode)."""
import torch
import torch.nn.functional as F

import mlp_ref as R

P, C_IN, C_MID, C_OUT = 37, 5, 7, 4
EPS, MOMENTUM = 1e-5, 0.1


def _layer():
    g = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x = rnd(P, C_IN)
    W1, b1 = rnd(C_MID, C_IN) * 0.5, rnd(C_MID) * 0.1
    gamma, beta = rnd(C_MID) * 0.5 + 1.0, rnd(C_MID) * 0.3
    gamma[2] = -gamma[2]                                           # (both signs)
    W2, G = rnd(C_OUT, C_MID) * 0.5, rnd(P, C_OUT)
    return x, W1, b1, gamma, beta, W2, G


def test_affine_block_is_training_mode_batch_norm():
    x, W1, b1, gamma, beta, _, _ = _layer()
    y = x @ W1.t() + b1
    rmean, rvar = torch.zeros(C_MID, dtype=torch.float64), torch.ones(C_MID, dtype=torch.float64)
    want = F.batch_norm(y, rmean, rvar, gamma, beta, True, MOMENTUM, EPS)
    mean, scale, b, invstd = R.affine_block(y.sum(0), (y * y).sum(0), P, gamma, beta, EPS)
    got = (y - mean) * scale + b
    assert R.rel(got, want) <= 1e-12
    assert R.rel(invstd, 1.0 / torch.sqrt(y.var(0, unbiased=False) + EPS)) <= 1e-12
    assert torch.equal(b, beta) and R.rel(scale, gamma * invstd) <= 1e-15
    rm, rv = R.running_stats(y.sum(0), (y * y).sum(0), P, MOMENTUM, torch.zeros(C_MID), torch.ones(C_MID))
    assert R.rel(rm, rmean) <= 1e-12 and R.rel(rv, rvar) <= 1e-12
    # the activation the cases stage is relu of that map (computed on the fp32 difference, rounded to fp32)
    yf = y.float()
    aff = torch.stack([mean, scale, b, invstd]).float()
    X, z = R.bn_relu(yf, aff)
    assert torch.equal(X, torch.clamp(z, min=0).float().double())
    assert R.rel(X, torch.relu(want)) <= 1e-6


def test_dy_statement_is_the_autograd_of_relu_batch_norm_linear():
    """dY = c0 dZ + q1 (y - mean) + q0 with the coefficient block derived as bn_coef_channel (csrc/bn_affine.h) derives it
    from the two reductions of the masked gradient, against fp64 autograd of relu(batch_norm(linear(x))): the gradient with
    respect to the pre-BN output, the weight and the bias of the linear layer, and BatchNorm's own dgamma / dbeta."""
    x, W1, b1, gamma, beta, W2, G = _layer()
    x = x.clone().requires_grad_(True)
    W1, b1, gamma, beta = (t.clone().requires_grad_(True) for t in (W1, b1, gamma, beta))
    y = x @ W1.t() + b1
    y.retain_grad()
    out = torch.relu(F.batch_norm(y, None, None, gamma, beta, True, MOMENTUM, EPS))
    ((out @ W2.t()) * G).sum().backward()

    yd = y.detach()
    mean, scale, b, invstd = R.affine_block(yd.sum(0), (yd * yd).sum(0), P, gamma.detach(), beta.detach(), EPS)
    dZ = ((G @ W2) * (out.detach() > 0))                           # the gradient behind the ReLU
    yhat = (yd - mean) * invstd
    r0, r1 = dZ.sum(0), (dZ * yhat).sum(0)
    coef = R.coef_block(r0, r1, P, gamma.detach(), mean, invstd)
    dY = R.dy_of(coef, dZ, yd)
    assert R.rel(dY, y.grad) <= 1e-12
    assert R.rel(dY.t() @ x.detach(), W1.grad) <= 1e-12
    assert R.rel(dY @ W1.detach(), x.grad) <= 1e-12
    assert R.rel(r1, gamma.grad) <= 1e-12 and R.rel(r0, beta.grad) <= 1e-12     # dgamma = red1, dbeta = red0 (include/pn2.h)
    # sum dY = 0 in training mode up to rounding (the conv bias has no gradient through BatchNorm): measured against sum |dY|
    assert float(dY.sum(0).abs().max()) <= 1e-12 * float(dY.abs().sum(0).max())


def test_fixed_cases_state_their_own_formulas():
    """The generators on the CPU at a small ragged shape: the statement returned with a case is the plain formula on the
    operands returned with it -- for the masked, the unmasked and the pooled form, with wide pitches, a sliced weight and
    scaled tail rows."""
    dev = torch.device("cpu")
    c, ref = R.fixed_layer_case(dev, P, C_MID, C_IN, 0, 3, masked=True, tail_from=32, w_mode="slice")
    assert c["ldc"] == 8 and c["ldp"] == 8 and c["ldw"] == C_IN + 3 and c["W"].data_ptr() == c["w_store"].data_ptr() + 12
    dZ = c["keep"][0]
    assert float(dZ[32:, :C_MID].abs().max()) > 4 * float(dZ[:32, :C_MID].abs().max())
    coef = c["coef"].view(4, 8)[:, :C_MID].double()
    aff = c["affp"].view(4, 8)[:, :C_IN]
    dY = coef[0] * dZ[:, :C_MID].double() + coef[1] * (c["Y"][:, :C_MID].double() - coef[3]) + coef[2]
    z = (c["Yp"][:, :C_IN] - aff[0]).double() * aff[1].double() + aff[2].double()
    assert R.rel(ref["dX"], (dY @ c["W"].double()) * (z > 0)) <= 1e-15
    assert R.rel(ref["dW"], dY.t() @ torch.relu(z).float().double()) <= 1e-15
    assert R.rel(ref["r0"], ref["dX"].sum(0)) <= 1e-15 and R.rel(ref["db"], dY.sum(0)) <= 1e-15

    c, ref = R.fixed_layer_case(dev, P, C_MID, C_IN, 0, 4, masked=False, ldc=16, ldp=12, w_mode="padded")
    assert c["affp"] is None and "r0" not in ref and c["Y"].shape == (P, 16) and c["Yp"].shape == (P, 12)
    assert float(c["Yp"][:, 8:].min()) > 1e29 and float(c["Yp"][:, C_IN:8].abs().max()) == 0.0
    assert float(c["w_store"][:, C_IN:].abs().max()) == 0.0 and c["ldw"] == 8
    coef = c["coef"].view(4, 8)[:, :C_MID].double()
    dY = coef[0] * c["keep"][0][:, :C_MID].double() + coef[1] * (c["Y"][:, :C_MID].double() - coef[3]) + coef[2]
    assert R.rel(ref["dX"], dY @ c["W"].double()) <= 1e-15 and R.rel(ref["dW"], dY.t() @ c["Yp"][:, :C_IN].double()) <= 1e-15

    Kp = 4
    c, ref = R.fixed_layer_case(dev, 36, C_MID, C_IN, Kp, 5, tail_from=32)
    dzp, arg = c["keep"]
    D = torch.zeros(36, C_MID, dtype=torch.float64)
    for gi in range(36 // Kp):
        for ch in range(C_MID):
            D[gi * Kp + int(arg[gi, ch]), ch] = float(dzp[gi, ch])
    coef = c["coef"].view(4, 8)[:, :C_MID].double()
    dY = coef[0] * D + coef[1] * (c["Y"][:, :C_MID].double() - coef[3]) + coef[2]
    assert R.rel(ref["db"], dY.sum(0)) <= 1e-15

    c, ref = R.fixed_forward_case(dev, P, C_IN, C_MID, 6, affine=True, ldy=16, tail_from=32)
    aff = c["aff"].view(4, 8)[:, :C_IN]
    act = torch.relu((c["X"][:, :C_IN] - aff[0]).double() * aff[1].double() + aff[2].double()).float().double()
    assert R.rel(ref["Y"], act @ c["W"].double().t() + c["bias"].double()) <= 1e-15
    assert R.rel(ref["s2"], (ref["Y"] ** 2).sum(0)) <= 1e-15
    c, ref = R.fixed_forward_case(dev, P, C_IN, C_MID, 7, affine=False, ldx=12)
    assert c["aff"] is None and R.rel(ref["Y"], c["X"][:, :C_IN].double() @ c["W"].double().t() + c["bias"].double()) <= 1e-15


def test_guards_see_a_stray_store():
    dev = torch.device("cpu")
    buf = R.guarded(5, 12, dev)
    buf[:5, :6] = 1.0
    buf[:5, 6:8] = 0.0
    R.check_guards(buf, 5, 6, "ok")
    for r, c_ in ((5, 0), (2, 8), (68, 11)):
        bad = buf.clone()
        bad[r, c_] = 0.0
        try:
            R.check_guards(bad, 5, 6, "stray")
        except AssertionError:
            continue
        raise AssertionError("a store at (%d, %d) went unnoticed" % (r, c_))
    tot = torch.arange(6, dtype=torch.float64).view(2, 3)
    assert torch.equal(R.replicate(tot).sum(0), tot) and R.replicate(tot).shape == (R.STAT_REPLICAS, 2, 3)
