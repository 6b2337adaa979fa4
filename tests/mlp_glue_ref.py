"""The yardstick of tests/test_mlp_routes_gpu.py: a plain torch shared MLP on rows [P, C] whose ReLU and arg-max DECISIONS can
be forced, the reader of the decisions a HIP ``_SharedMLP`` node made, the bound the gradients are held to, and a hand-written
backward of the same function in which tests/test_mlp_glue_ref_cpu.py plants wiring faults.

Why forced decisions: a pre-activation within a rounding of 0, or two rows of a group within a rounding of each other, fall
one way in fp32 and the other in fp64, and one such flip moves a weight gradient by ~1e-3 of its largest entry.  With the
device's own decisions forced (``bn(.) * mask`` in place of ReLU, a gather at the recorded row in place of ``max``) the function
is smooth in everything else, and an fp32 evaluation sits ~1e-6 from the fp64 one: a bound of 5e-5 then separates rounding from
a wrong operand.  Nothing here imports the package or the oracle.
"""
import torch
import torch.nn.functional as F

FORCED_TOL = 5e-5            # tests/test_parity_stages_gpu.py: every gradient tensor against fp64 with the decisions forced
FACTOR = 4.0                 # tests/test_mlp_gpu.py (_check_shared_mlp): what it grants over plain torch fp32 on the same input
FLIP_SLACK = 2e-2            # ... and what it allows from 2048 rows on, where a decision may flip

# (P, pool, channels) of the tests/test_mlp_routes_gpu.py cases whose fp64 gradients test_mlp_glue_ref_cpu.py plants faults in
FAULT_SHAPES = {"streamed-dense": (1041, 0, [20, 32, 13]), "streamed-pooled": (2064, 16, [9, 32, 64]), "pair": (8192, 0, [128, 128, 128]),
                "resident-dense": (64 * 16 + 17, 0, [12, 64, 64, 96]), "resident-pooled": (33 * 64, 64, [32, 64, 128])}


def make_case(P, pool, chans, seed, training=True):
    """Operands of one stack on the CPU in float32: rows [P, C_0] with non-zero means, per layer (W [co, ci], bias [co]) and
    (gamma, beta, running_mean, running_var, eps) -- gamma of both signs with every fifth one exactly 0, beta in (-1, 1), as
    test_shared_mlp_negative_and_zero_gamma draws them; in eval mode running statistics away from (0, 1)."""
    gen = torch.Generator().manual_seed(seed)
    rows = torch.randn(P, chans[0], generator=gen) * 2 + 0.5
    weights, bn_params = [], []
    for ci, co in zip(chans[:-1], chans[1:]):
        bound = 1.0 / ci ** 0.5
        weights.append(((torch.rand(co, ci, generator=gen) * 2 - 1) * bound, (torch.rand(co, generator=gen) * 2 - 1) * bound))
        gamma = torch.rand(co, generator=gen) * 3 - 1.5
        gamma[::5] = 0.0
        beta = torch.rand(co, generator=gen) * 2 - 1
        rmean, rvar = torch.zeros(co), torch.ones(co)
        if not training:
            rmean, rvar = torch.rand(co, generator=gen) * 0.6 - 0.3, torch.rand(co, generator=gen) * 1.5 + 0.5
        bn_params.append((gamma, beta, rmean, rvar, 1e-5))
    return rows, weights, bn_params


def forced_mlp(rows64, weights, bn_params, pool, training, decisions, dtype):
    """conv -> BatchNorm (batch statistics in training) -> ReLU per layer on rows [P, C], then the max over ``pool`` consecutive
    rows, in ``dtype``.  ``decisions`` None: the function as it stands.  Otherwise {"masks": [bool [P, C_l]], "arg": int64
    [P / pool, C_L] or None}: ``bn(.) * mask`` in place of ReLU and a gather at the recorded row in place of max.
    -> (output, made): ``made`` holds the decisions this evaluation would make itself ("masks", "arg") and per layer the batch
    mean and unbiased variance of the pre-BN activation ("stats": what the running statistics are updated with)."""
    y = rows64.to(dtype)
    made = {"masks": [], "arg": None, "stats": []}
    for l, ((w, b), (gamma, beta, rmean, rvar, eps)) in enumerate(zip(weights, bn_params)):
        y = F.linear(y, w.to(dtype), b.to(dtype))
        made["stats"].append((y.detach().mean(0), y.detach().var(0, unbiased=True)))
        mean, var = (y.mean(0), y.var(0, unbiased=False)) if training else (rmean.to(dtype), rvar.to(dtype))
        z = (y - mean) / torch.sqrt(var + eps) * gamma.to(dtype) + beta.to(dtype)
        made["masks"].append(z.detach() > 0)
        y = torch.relu(z) if decisions is None else z * decisions["masks"][l].to(dtype)
    if pool:
        y = y.view(-1, pool, y.shape[1])
        if decisions is None:
            y, arg = y.max(1)
        else:
            arg = decisions["arg"]
            y = y.gather(1, arg.unsqueeze(1)).squeeze(1)
        made["arg"] = arg.detach()
    return y, made


def mlp_node(out):
    """The _SharedMLP autograd node behind ``out`` (``out`` itself, or a view of it)."""
    fn = out.grad_fn
    while fn is not None and type(fn).__name__ != "_SharedMLPBackward":
        fn = fn.next_functions[0][0] if fn.next_functions else None
    assert fn is not None, "no _SharedMLP node behind this tensor"
    return fn


def decisions_of(out):
    """The decisions of the HIP node behind ``out`` in row layout, read from its saved tensors before the backward releases
    them: per layer the sign of (Y - mean) * scale + beta from the saved affine block -- Y - mean rounded to fp32 first, as in the
    kernels; the product of two fp32 values is exact in fp64, so the sign is the kernels' own -- and the saved arg-max.  A last
    layer that ran without its output (Ys[-1] is None) has decisions at the recorded arg-max rows only, where the decision is
    "pooled output > 0": its mask holds exactly those ("last_at_arg_only")."""
    fn = mlp_node(out)
    chans, pool, _training, P = fn.meta
    saved = fn.saved_tensors
    L = len(chans) - 1
    pooled_out, arg = saved[1], saved[2]
    Ys, affs = saved[3:3 + L], saved[3 + L:3 + 2 * L]
    K = pool if pool else 1
    G = P // K
    masks = []
    for l in range(L):
        C = chans[l + 1]
        ld = (C + 3) & ~3
        mean, scale, beta = affs[l][:C], affs[l][ld:ld + C], affs[l][2 * ld:2 * ld + C]
        if Ys[l] is None:
            assert pool and l == L - 1
            m = torch.zeros(G, K, C, dtype=torch.bool, device=pooled_out.device)
            m.scatter_(1, arg[:, :C].long().unsqueeze(1), (pooled_out[:, :C] > 0).unsqueeze(1))
            masks.append(m.view(P, C))
        else:
            masks.append(((Ys[l][:, :C] - mean).double() * scale.double() + beta.double()) > 0)
    return {"masks": masks, "arg": arg[:, :chans[-1]].long().contiguous() if pool else None,
            "last_at_arg_only": bool(pool and Ys[-1] is None), "carry": (pooled_out[:, :chans[-1]] > 0) if pool else None}


def decisions_differing(dec, made):
    """How many of the device's decisions ``dec`` (decisions_of) differ from those an evaluation made itself (forced_mlp's
    ``made``): ReLU mask positions, plus arg-max positions among those that carry a gradient (output > 0)."""
    n = 0
    for l, (a, b) in enumerate(zip(dec["masks"], made["masks"])):
        if dec.get("last_at_arg_only") and l == len(dec["masks"]) - 1:
            G, C = dec["arg"].shape
            idx = dec["arg"].unsqueeze(1)
            n += int((a.view(G, -1, C).gather(1, idx) != b.view(G, -1, C).gather(1, idx)).sum())
        else:
            n += int((a != b).sum())
    if dec["arg"] is not None:
        carry = dec["carry"] if dec.get("carry") is not None else torch.ones_like(dec["arg"], dtype=torch.bool)
        n += int(((dec["arg"] != made["arg"]) & carry).sum())
    return n


def prefill_like(ref):
    """What a ``.grad`` holds before a backward under direct accumulation: known, non-zero, of the size of the gradient that is
    added to it (between 0.5 and 1 of its largest entry; 1 .. 2 where the gradient is zero), so that a kernel that overwrites
    and one that skips the tensor both show."""
    scale = float(ref.abs().max()) or 2.0
    ramp = torch.linspace(0.5, 1.0, ref.numel(), dtype=ref.dtype, device=ref.device).view(ref.shape)
    return scale * ramp


def grad_bound(ref, t32):
    """max(5e-5 max|ref|, 4 max|t32 - ref|): ``t32`` is the same forced function in stock torch float32."""
    ref = ref.double()
    return max(FORCED_TOL * float(ref.abs().max()), FACTOR * float((t32.double().to(ref.device) - ref).abs().max()))


def ratio_to_bound(got, ref, t32):
    """max|got - ref| over grad_bound; a reference that is exactly zero asks for exact zeros (ratio 0 or inf)."""
    ref = ref.double()
    err = float((got.double().to(ref.device) - ref).abs().max())
    if float(ref.abs().max()) == 0.0:
        return 0.0 if err == 0.0 else float("inf")
    return err / grad_bound(ref, t32)


# ------------------------------------------------------------------------------------------ the backward written out, with faults

def manual_backward(rows, weights, bn_params, pool, decisions, grad_out, fault=None, ld_slice=None):
    """Gradients of ``(forced_mlp(...) * grad_out).sum()`` in training mode, float64, as the kernels form them: per layer
    dY = c0 dZ + q1 (y - mean) + q0 from the two reductions (dbeta = sum dZ, dgamma = sum dZ xhat), dW = dY^T x, dX = dY W
    masked by the layer below.  -> {"rows", "W<l>", "gamma<l>", "beta<l>"}.

    ``fault`` plants one wiring error of the kind the autograd glue could make:
      "q1-next-layer"   layer l's q1 is formed from layer l+1's reductions (channel c reads channel c mod C_{l+1})
      "swap-dgamma"     dgamma / dbeta of layers 0 and 1 are handed back swapped (padded / cut to the other's length)
      "dw-tail-64"      every dW misses the contribution of the last 64 rows
      "pitch"           (pooled) grad_out is a column slice at pitch ``ld_slice`` of a wider matrix but is read at pitch C_L
    """
    dt = torch.float64
    x = rows.to(dt)
    L, P = len(weights), rows.shape[0]
    saved = []
    for l, ((w, b), (gamma, beta, _rm, _rv, eps)) in enumerate(zip(weights, bn_params)):
        y = x @ w.to(dt).t() + b.to(dt)
        mean, invstd = y.mean(0), 1.0 / torch.sqrt(y.var(0, unbiased=False) + eps)
        xhat = (y - mean) * invstd
        mask = decisions["masks"][l].to(dt)
        saved.append((x, xhat, invstd, mask))
        x = (xhat * gamma.to(dt) + beta.to(dt)) * mask
    g = grad_out.to(dt)
    if pool and fault == "pitch":
        G, C = g.shape
        wide = torch.full((G, ld_slice), 7.0, dtype=dt)           # what the neighbouring slices of the wide matrix hold
        wide[:, 64:64 + C] = g
        g = wide.flatten()[64:64 + G * C].view(G, C)               # rows at pitch C from the slice's first element
    if pool:
        full = torch.zeros(P // pool, pool, g.shape[1], dtype=dt)
        full.scatter_(1, decisions["arg"].unsqueeze(1), g.unsqueeze(1))
        g = full.view(P, -1)
    out, red_above = {}, None
    for l in range(L - 1, -1, -1):
        x, xhat, invstd, mask = saved[l]
        gamma = bn_params[l][0].to(dt)
        dz = g * mask
        dbeta, dgamma = dz.sum(0), (dz * xhat).sum(0)
        r1 = dgamma
        if fault == "q1-next-layer" and red_above is not None:
            r1 = red_above[torch.arange(dgamma.numel()) % red_above.numel()]
        red_above = dgamma
        c0 = gamma * invstd
        dy = c0 * (dz - dbeta / P - xhat * (r1 / P))
        keep = slice(0, P - 64) if fault == "dw-tail-64" else slice(None)
        out["W%d" % l], out["gamma%d" % l], out["beta%d" % l] = dy[keep].t() @ x[keep], dgamma, dbeta
        g = dy @ weights[l][0].to(dt)
    out["rows"] = g
    if fault == "swap-dgamma":
        for k in ("gamma", "beta"):
            a, b = out[k + "0"], out[k + "1"]
            fit = lambda t, n: t[torch.arange(n) % t.numel()]
            out[k + "0"], out[k + "1"] = fit(b, a.numel()), fit(a, b.numel())
    return out
