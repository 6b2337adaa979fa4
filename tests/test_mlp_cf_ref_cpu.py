"""tests/mlp_cf_ref.py on the CPU, without the library: (1) its statements are fp64 autograd of conv + training-mode BatchNorm +
ReLU + max-pool; (2) a float32 emulation of the closed forms AS THE KERNELS COMPUTE THEM passes every bound the GPU file
(tests/test_mlp_cf_seams_gpu.py) holds the kernels to, on every case family, so the bounds are reachable by correct float32
arithmetic; (3) ten mutants of that emulation -- the ways these kernels can be subtly wrong -- each miss a bound on every case
they change.

The emulation (csrc/mlp_res.hip, "pooled last layer from its INPUT"; csrc/mlp.hip, "first-layer dW, closed form"):
W2 = [diag(c0) W ; W^T diag(q1) W] and h = (q1 (b - mean) + q0)^T W in fp64, rounded to float32; dX = ([D | X] W2 + h) o mask in
float32, odd 32-row chunks multiplied negated and flipped back before h joins; T = X^T [D | X] and sx = sum x in float32 per
workgroup slab (chunks dealt round-robin to `grid` workgroups), the slabs summed in fp64; dW = c0 o (D^T X) + q1 o (W Gram + (b -
mean) sx^T) + q0 sx^T in fp64, rounded to float32 and added to dW's contents.  The first-layer form: part = dZ^T x in float32,
the moments S and s in fp64, the same finish over the N real columns (part accumulated as the kernel's waves do: _part_mfma).
"""
import pytest
import torch
import torch.nn.functional as F

import mlp_cf_ref as C
import mlp_ref as R

DEV = torch.device("cpu")
RM, GRIDS = 1024, (8, 7)                                            # a stand-in threshold and two grid caps (even; odd: sign alternation inside a workgroup)
SHAPES = ((128, 96), (128, 64))
MUTANTS_CF = ("last-chunk-dropped", "chunk-counted-twice", "odd-chunks-not-un-negated", "arg-compared-without-kbase", "ldo-taken-as-c-out",
              "gram-not-mirrored", "h-omitted", "b-mean-sx-omitted", "slab-sum-stops-at-a-multiple-of-4")
MUTANTS_FIRST = ("b-mean-sx-omitted", "pad-columns-read-as-data")


# =============================================================================================== (1) the statements are autograd

def _pooled_layer(P, ci, co, Kp, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    Yp = rnd(P, ci) * 1.5 + 0.3
    aff = torch.stack([rnd(ci) * 0.2, (rnd(ci) * 0.5).abs() + 0.3, rnd(ci) * 0.3, (rnd(ci) * 0.2).abs() + 0.8])
    aff[1, ::3] *= -1.0
    W, b = rnd(co, ci) * 0.4, rnd(co) * 0.1
    gamma, beta = rnd(co) * 0.5 + 1.0, rnd(co) * 0.3
    gamma[1] = -gamma[1]
    return Yp, aff, W, b, gamma, beta, rnd(P // Kp, co)


@pytest.mark.parametrize("P,Kp", [(48, 4), (64, 32), (40, 1)])
def test_bwd_cf_statement_is_autograd_of_conv_batchnorm_relu_maxpool(P, Kp):
    """layer_statement on the self-consistent block (D scattered from the pooled gradient and the arg-max rows, mean / invstd the
    true statistics of Y) against fp64 autograd of max_k relu(batch_norm(relu(bn(prev_Y)) W^T + b)): the gradient with respect to
    prev_Y (the masked dX times the previous scale), W, and BatchNorm's dgamma / dbeta (= the two reductions)."""
    ci, co = 6, 5
    Yp, aff, W, b, gamma, beta, Gout = _pooled_layer(P, ci, co, Kp, 100 + P)
    Yp, W, b, gamma, beta = (t.clone().requires_grad_(True) for t in (Yp, W, b, gamma, beta))
    z = (Yp - aff[0]) * aff[1] + aff[2]
    X = torch.relu(z)
    Y = X @ W.t() + b
    act = torch.relu(F.batch_norm(Y, None, None, gamma, beta, True, 0.1, C.EPS))
    out, arg = act.view(P // Kp, Kp, co).max(1)
    (out * Gout).sum().backward()

    dzp = Gout * (out.detach() > 0)
    D = C.scatter_rows(dzp, arg, Kp)
    Xd, Wd, bd = X.detach(), W.detach(), b.detach()
    block = C.self_block(D, Xd @ Wd.t() + bd, gamma.detach())
    xhat = (Yp.detach() - aff[0]) * aff[3]
    st = C.layer_statement(D, block, Wd, bd, Xd, z.detach() > 0, xhat)
    assert R.rel(st["dX"] * aff[1], Yp.grad) <= 1e-12
    assert R.rel(st["dW"], W.grad) <= 1e-12
    mean, invstd = C.true_stats(st["Y"])
    assert R.rel((D * (st["Y"] - mean) * invstd).sum(0), gamma.grad) <= 1e-12 and R.rel(D.sum(0), beta.grad) <= 1e-12
    # the cancellation a real BatchNorm backward has, against the sums of the magnitudes: sum dY = 0, and sum dY yhat = 0 up to
    # the eps under the root (exactly c0 r1 eps invstd^2)
    dY, yhat = st["dY"], (st["Y"] - mean) * invstd
    assert float(dY.sum(0).abs().max()) <= 1e-12 * float(dY.abs().sum(0).max())
    left = block[0] * (D * yhat).sum(0) * C.EPS * invstd * invstd
    assert float(((dY * yhat).sum(0) - left).abs().max()) <= 1e-12 * float((dY * yhat).abs().sum(0).max())
    assert float((dY * yhat).sum(0).abs().max()) <= 1e-3 * float((dY * yhat).abs().sum(0).max())
    # and the reductions the statement hands the previous layer are that layer's dbeta / dgamma
    assert R.rel(st["r0"], st["dX"].sum(0)) <= 1e-15 and R.rel(st["r1"], (st["dX"] * xhat).sum(0)) <= 1e-15


@pytest.mark.parametrize("P,N,M", [(37, 5, 16), (3, 3, 16), (130, 12, 32), (64, 1, 16)])
def test_first_layer_statement_is_autograd_of_conv_batchnorm(P, N, M):
    """first_dw_statement (the closed form of include/pn2.h: c0 dZ^T x + q1 (W S + (b - mean) s^T) + q0 s^T) on the self-consistent
    block against fp64 autograd of batch_norm(x W^T + b) under a fixed output gradient dZ, and against the textbook dY^T x."""
    g = torch.Generator().manual_seed(P + N)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x = rnd(P, N) * torch.linspace(0.3, 2.0, N, dtype=torch.float64) + torch.linspace(-1.0, 3.0, N, dtype=torch.float64)
    W, b = (rnd(M, N) * 0.3).requires_grad_(True), rnd(M) * 0.1
    gamma, dZ = rnd(M) * 0.5 + 1.0, rnd(P, M)
    (F.batch_norm(x @ W.t() + b, None, None, gamma, torch.zeros(M, dtype=torch.float64), True, 0.1, C.EPS) * dZ).sum().backward()
    Wd = W.detach()
    block = C.self_block(dZ, x @ Wd.t() + b, gamma)
    closed = C.first_dw_statement(dZ.t() @ x, block, Wd, b, x)
    scale = max(float(closed.abs().max()), float((block[0][:, None] * (dZ.t() @ x)).abs().max()))     # (few rows: nearly everything cancels)
    assert float((closed - W.grad).abs().max()) <= 1e-12 * scale
    assert float((closed - C.layer_statement(dZ, block, Wd, b, x)["dW"]).abs().max()) <= 1e-12 * scale


def test_the_chained_first_layer_statement_of_first_case():
    """first_case's dW0 is first_dw_statement on part = (the second layer's masked dX)^T x0, general in N0 and ld0; its inputs
    obey the buffer rules."""
    for N0, ld0 in ((3, 12), (9, 16), (12, 12)):
        c, ref = C.first_case(DEV, 128, 96, 64, N0, ld0, 5, wide=True)
        x0 = c["X0"][:, :N0].double()
        assert ref["dW0"].shape == (64, N0)
        assert R.rel(ref["dW0"], C.first_dw_statement(ref["dX"].t() @ x0, c["coef0"].view(4, 64), c["W0"], c["b0"], x0)) <= 1e-15
        assert float(c["X0"][:, N0:12].abs().max() if N0 < 12 else 0.0) == 0.0 and bool(torch.isnan(c["X0"][:, 12:]).all())
        assert bool(torch.isnan(c["Y"][:, 96:]).all()) and bool(torch.isnan(c["Yp"][:, 64:]).all()) and bool(torch.isnan(c["w0_store"][:, N0:]).all())


# =============================================================================================== (2) the emulation

def _d_image(c, P, co, mutant):
    """float32 D [P, co] as split_bwd_cf_kernel's staging selects it: row p of group p >> kshift takes dZp[g, ch] where
    arg[g, ch] == kbase + row-in-chunk."""
    Kp, G = c["Kp"], P // c["Kp"]
    dzp, arg = c["dzp"], c["arg"]
    if mutant == "ldo-taken-as-c-out":
        dzp, arg = dzp.reshape(-1)[:G * co].view(G, co), arg.reshape(-1)[:G * co].view(G, co)
    dzr, ar = dzp[:, :co].repeat_interleave(Kp, 0), arg[:, :co].repeat_interleave(Kp, 0)
    k = torch.arange(P) % (32 if mutant == "arg-compared-without-kbase" else Kp)
    return torch.where(ar == k[:, None], dzr, torch.zeros(()))


def _finish(T, sx, cf, W, b, mutant):
    """cf_finish_kernel on the summed slab (fp64): row i of T = [X^T D | Gram], dot = sum_j W[c, j] T[i, Co + j]."""
    co = W.shape[0]
    c0, q1, q0, mu = cf
    bm = torch.zeros_like(b) if mutant == "b-mean-sx-omitted" else b - mu
    return c0[:, None] * T[:, :co].t() + q1[:, None] * (W @ T[:, co:].t() + bm[:, None] * sx[None, :]) + q0[:, None] * sx[None, :]


def emulate_bwd_cf(c, ref, P, co, ci, grid, mutant=None):
    """{dX, dW (the increment), r0, r1} of pn2_conv1x1_bwd_cf in emulated float32 (module docstring) on `grid` workgroups."""
    cf, W, b = c["coef"].view(4, co).double(), c["W"].double(), c["bias"].double()
    c0, q1, q0, mu = cf
    W2 = torch.cat([c0[:, None] * W, W.t() @ (q1[:, None] * W)]).float()                 # cf_prep_kernel
    h = ((q1 * (b - mu) + q0) @ W).float()
    if mutant == "h-omitted":
        h = torch.zeros_like(h)
    X = ref["X"].float()
    A = torch.cat([_d_image(c, P, co, mutant), X], 1)
    chunks = P // 32
    grid = min(grid, chunks)
    odd = (torch.arange(P) // 32 % 2 == 1)[:, None]
    prod = A @ W2                                                   # (an odd chunk: -((-A) W2), the same bits)
    if mutant == "odd-chunks-not-un-negated":
        prod = torch.where(odd, -prod, prod)
    dX = torch.where(ref["mask"], prod + h, torch.zeros(()))
    count = torch.ones(chunks)
    if mutant == "last-chunk-dropped":
        count[-1] = 0
        dX[-32:] = C.NAN                                            # (never written: the guard pattern)
    if mutant == "chunk-counted-twice":
        count[chunks // 2] = 2
    rw = count.repeat_interleave(32)[:, None]
    xhat = ((c["Yp"][:, :ci] - c["affp"][:ci]) * c["affp"][3 * ci:]).float()
    nslab = grid - grid % 4 if mutant == "slab-sum-stops-at-a-multiple-of-4" else grid
    T, sx = torch.zeros(ci, co + ci, dtype=torch.float64), torch.zeros(ci, dtype=torch.float64)
    r0, r1 = torch.zeros(ci, dtype=torch.float64), torch.zeros(ci, dtype=torch.float64)
    live = torch.where(rw > 0, dX, torch.zeros(()))
    for w in range(grid):
        rows = (torch.arange(w, chunks, grid)[:, None] * 32 + torch.arange(32)[None, :]).reshape(-1)
        Xw = X[rows] * rw[rows]
        r0 += (live[rows] * rw[rows]).sum(0).double()
        r1 += (live[rows] * rw[rows] * xhat[rows]).sum(0).double()
        if w < nslab:
            T += (Xw.t() @ A[rows]).double()
            sx += Xw.sum(0).double()
    if mutant == "gram-not-mirrored":
        for i in range(ci // 32):
            for j in range(i):
                T[32 * i:32 * i + 32, co + 32 * j:co + 32 * j + 32] = 0.0
    return {"dX": dX, "dW": _finish(T, sx, cf, W, b, mutant).float(), "r0": r0, "r1": r1}


def _first_finish(part, X, N, coef0, w_store, b0, mutant):
    """wgrad_first_cf_kernel's last workgroup: the moments of the N real columns (fp64 from the first product on) and the closed
    form in fp64, rounded to float32."""
    n = min(N + 3, X.shape[1]) if mutant == "pad-columns-read-as-data" else N       # (w_store is N + 3 wide)
    x = X[:, :n].double()
    S, s = x.t() @ x, x.sum(0)
    c0, q1, q0, mu = coef0.double()
    bm = torch.zeros_like(mu) if mutant == "b-mean-sx-omitted" else b0.double() - mu
    dW = c0[:, None] * part[:, :n].double() + q1[:, None] * (w_store[:, :n].double() @ S + bm[:, None] * s[None, :]) + q0[:, None] * s[None, :]
    return dW.float()[:, :N]


def _part_mfma(dZ, X, grid_cap):
    """float32 dZ^T X as wgrad_first_cf_kernel accumulates it: every wave of min(cdiv(P, 512), grid_cap) four-wave workgroups
    owns runs of 8 x 4 rows and adds one 4-row product per MFMA into its float32 accumulator (the 4-term dot taken as exact,
    one rounding per step); the waves of a workgroup, the workgroups of a replica and the eight replicas are added in float32."""
    P, grid = dZ.shape[0], max(1, min(-(-dZ.shape[0] // 512), grid_cap))
    A = 4 * grid
    trips = -(-P // (A * 32))
    pad = lambda t: torch.cat([t, torch.zeros(trips * A * 32 - P, t.shape[1])]).view(trips, A, 8, 4, t.shape[1]).double()
    z, x = pad(dZ), pad(X)
    acc = torch.zeros(A, dZ.shape[1], X.shape[1])
    for t in range(trips):
        for u in range(8):
            acc = (acc.double() + torch.einsum("akm,akn->amn", z[t, :, u], x[t, :, u])).float()
    wg = acc.view(grid, 4, *acc.shape[1:])
    wg = ((wg[:, 0] + wg[:, 1]) + wg[:, 2]) + wg[:, 3]
    rep = torch.zeros(8, *acc.shape[1:])
    for b in range(grid):
        rep[b % 8] += wg[b]
    out = torch.zeros_like(rep[0])
    for r in range(8):
        out += rep[r]
    return out


def emulate_wgrad_cf(c, M, N, mutant=None, grid_cap=8):
    part = torch.zeros(M, c["X"].shape[1])
    part[:, :N] = _part_mfma(c["dZ"][:, :M], c["X"][:, :N], grid_cap)
    return _first_finish(part, c["X"], N, c["coef"].view(4, M), c["w_store"], c["bias"], mutant)


def emulate_first(c, ref, co, ci, mutant=None):
    """{dW, r0, r1, dW0} of pn2_conv1x1_bwd_first + pn2_conv1x1_wgrad_cf(dZ = NULL): dY per row in float32, dX = (dY W) o mask and
    part = dX^T X0 over the twelve columns the kernel reads."""
    cf, ap = c["coef"].view(4, co), c["affp"].view(4, ci)
    dY = cf[0] * c["keep"][0][:, :co] + cf[1] * (c["Y"][:, :co] - cf[3]) + cf[2]
    X, z = R.bn_relu(c["Yp"][:, :ci], ap)
    dX = torch.where(z > 0, dY @ c["W"], torch.zeros(()))
    xhat = (c["Yp"][:, :ci] - ap[0]) * ap[3]
    part = torch.zeros(ci, c["X0"].shape[1])
    part[:, :12] = dX.t() @ c["X0"][:, :12]
    return {"dW": dY.t() @ X.float(), "r0": dX.sum(0), "r1": (dX * xhat).sum(0),
            "dW0": _first_finish(part, c["X0"], c["N0"], c["coef0"].view(4, ci), c["w0_store"], c["b0"], mutant)}


# =============================================================================================== (2), (3) the bounds and the mutants

def _misses(got, ref, keys, kind, f32):
    """The tensors of `keys` that miss their bound (a NaN misses)."""
    out = []
    for k in keys:
        if k == "dX" and "head" in ref:
            e = max(R.rel(got[k][lo:hi], ref[k][lo:hi]) for lo, hi in ((0, ref["head"]), (ref["head"], ref[k].shape[0])))
            e32 = max(R.rel(f32[k][lo:hi], ref[k][lo:hi]) for lo, hi in ((0, ref["head"]), (ref["head"], ref[k].shape[0])))
        else:
            e, e32 = R.rel(got[k], ref[k]), (R.rel(f32[k], ref[k]) if f32 is not None else 0.0)
        if not e <= C.bound(kind, e32):
            out.append((k, e))
    return out


def _same(a, b):
    return all(torch.equal(torch.nan_to_num(a[k].double(), nan=1e300), torch.nan_to_num(b[k].double(), nan=1e300)) for k in a)


def _cf_cases():
    for co, ci in SHAPES:
        for grid in GRIDS:
            for name, (P, Kp, kw, _) in C.bwd_cf_table(RM, grid, co, ci).items():
                yield "%dx%d-g%d-%s" % (co, ci, grid, name), co, ci, grid, P, Kp, kw
            for n in C.SMALL_N:
                yield "%dx%d-g%d-small-%s" % (co, ci, grid, n), co, ci, grid, 32 * C.small_n(n, grid), 32, {}


CF_CASES = list(_cf_cases())
assert len(CF_CASES) == 2 * len(GRIDS) * (len(C.BWD_CF_NAMES) + len(C.SMALL_N))


def test_emulated_bwd_cf_is_inside_every_bound_and_every_mutant_outside():
    changed = {m: 0 for m in MUTANTS_CF}
    worst = {}
    for i, (name, co, ci, grid, P, Kp, kw) in enumerate(CF_CASES):
        c, ref = C.bwd_cf_case(DEV, P, co, ci, Kp, 9000 + i, **kw)
        if "tail_from" in kw:
            ref["head"] = kw["tail_from"]
        keys = ("dX", "dW", "r0", "r1")
        base = emulate_bwd_cf(c, ref, P, co, ci, grid)
        if kw.get("zero_dzp"):
            assert all(float(base[k].abs().max()) == 0.0 for k in keys), name       # exactly zero, dW's increment included
            continue                                                                # (a zero reference has no scale: nothing else to hold)
        if kw.get("dead") is not None:
            assert float(base["dX"][:, kw["dead"]].abs().max()) == 0.0 and float(base["dW"][:, kw["dead"]].abs().max()) == 0.0, name
        bad = _misses(base, ref, keys, ref["kind"], ref["f32"])
        assert not bad, (name, bad)
        for k in keys:
            worst[k] = max(worst.get(k, 0.0), R.rel(base[k], ref[k]))
        for m in MUTANTS_CF:
            got = emulate_bwd_cf(c, ref, P, co, ci, grid, m)
            if _same(got, base):
                continue
            changed[m] += 1
            assert _misses(got, ref, keys, ref["kind"], ref["f32"]), "mutant %s passes case %s" % (m, name)
    print("emulated bwd_cf, largest errors: " + "  ".join("%s %.2e" % kv for kv in worst.items()), " cases changed per mutant:", changed)
    assert all(n >= 4 for n in changed.values()), changed


def _first_cases():
    i = 0
    for co, ci in ((96, 64), (64, 64)):
        for N0 in (1, 3, 6, 9, 12):
            for ld0 in (12, 16):
                i += 1
                yield co, ci, N0, ld0, 64 * (3 + i % 5), None
        yield co, ci, 12, 12, RM + 64, RM


def test_emulated_bwd_first_is_inside_every_bound_and_every_mutant_outside():
    changed = {m: 0 for m in MUTANTS_FIRST}
    for i, (co, ci, N0, ld0, P, tail) in enumerate(_first_cases()):
        c, ref = C.first_case(DEV, P, co, ci, N0, ld0, 9500 + i, tail_from=tail, wide=bool(i % 2))
        keys = ("dW", "r0", "r1", "dW0")
        base = emulate_first(c, ref, co, ci)
        assert not _misses(base, ref, keys, "random", None), (co, ci, N0, ld0, _misses(base, ref, keys, "random", None))
        for m in MUTANTS_FIRST:
            got = emulate_first(c, ref, co, ci, m)
            if _same(got, base):
                continue
            changed[m] += 1
            assert _misses(got, ref, keys, "random", None), "mutant %s passes %s" % (m, (co, ci, N0, ld0))
    assert all(n >= 4 for n in changed.values()), changed


WGRAD_MS, WGRAD_NS, WGRAD_PS = tuple(range(16, 129, 16)), (1, 3, 4, 5, 9, 12, 15), (1, 3, 127, 128, 129, 511, 512, 513)


def test_emulated_wgrad_cf_is_inside_every_bound_and_every_mutant_outside():
    changed = {m: 0 for m in MUTANTS_FIRST}
    i = 0
    for M in WGRAD_MS:
        for N in WGRAD_NS:
            for P in WGRAD_PS[(M // 16 + N) % 2::2]:                # (half of the row counts per shape here; the GPU file runs all)
                for kind in C.wgrad_cf_kinds(P, N):
                    i += 1
                    c, ref = C.wgrad_cf_case(DEV, P, M, N, R.round4(N) + 4 * (i % 2), M + 4, 9700 + i, coef=kind)
                    assert R.rel(ref["closed"], ref["dW"]) <= 1e-11
                    base = {"dW": emulate_wgrad_cf(c, M, N)}
                    assert not _misses(base, ref, ("dW",), kind, ref["f32"]), (M, N, P, kind, _misses(base, ref, ("dW",), kind, ref["f32"]))
                    for m in MUTANTS_FIRST:
                        got = {"dW": emulate_wgrad_cf(c, M, N, m)}
                        if _same(got, base):
                            continue
                        changed[m] += 1
                        assert _misses(got, ref, ("dW",), kind, ref["f32"]), "mutant %s passes %s" % (m, (M, N, P, kind))
    assert all(n >= 4 for n in changed.values()), changed


def test_the_operands_obey_the_buffer_rules():
    c, ref = C.bwd_cf_case(DEV, 128, 128, 96, 64, 3, ldo=136, ldp=100, ldw=99, arg_mode="planted", dead=5)
    assert bool(torch.isnan(c["dzp"][:, 128:]).all()) and bool((c["arg"][:, 128:] > 1 << 20).all()) and bool(torch.isnan(c["Yp"][:, 96:]).all())
    assert bool(torch.isnan(c["w_store"][:, 96:]).all()) and c["W"].data_ptr() == c["w_store"].data_ptr()
    assert bool((c["arg"][:, 0] == 31).all()) and bool((c["arg"][:, 1] == 32).all())
    assert float(ref["X"][:, 5].abs().max()) == 0.0 and not bool(ref["mask"][:, 5].any())
    assert float(ref["X"].abs().max()) > 0 and bool((ref["X"] == ref["X"].float().double()).all())
    c, ref = C.wgrad_cf_case(DEV, 9, 16, 5, 12, 20, 4)
    assert bool(torch.isnan(c["X"][:, 5:]).all()) and bool(torch.isnan(c["dZ"][:, 16:]).all()) and bool(torch.isnan(c["w_store"][:, 5:]).all())


def test_a_self_consistent_block_on_one_input_column_leaves_a_null_gradient():
    """Why mlp_cf_ref.wgrad_cf_kinds gives the self-consistent block to N >= 3 only.  With ONE input column every column of Y is an
    affine function of it, BatchNorm removes exactly that, and dW is not a cancelled sum with a scale of its own but the residue
    of the eps under the root: dW[c] = sum dY x = (sum dY (y - mean)) / w = c0 r1 eps invstd / w -- here 1e-3 .. 1e-1 of its
    terms, where a float32 evaluation and its float32 reference are two roundings of nothing (the emulation above lands on either
    side of 4 e32 from seed to seed)."""
    for seed in range(4):
        c, ref = C.wgrad_cf_case(DEV, 129, 32, 1, 4, 36, seed, coef="self")
        x, D, w = c["X"][:, :1].double(), c["dZ"][:, :32].double(), c["W"].double()[:, 0]
        Y = x @ c["W"].double().t() + c["bias"].double()
        mean, invstd = C.true_stats(Y)
        gamma = c["coef"].view(4, 32)[0].double() / invstd
        block = C.self_block(D, Y, gamma)                           # (in fp64: the statement of the case is on its float32 rounding)
        null = block[0] * (D * (Y - mean) * invstd).sum(0) * C.EPS * invstd / w
        dW = C.layer_statement(D, block, c["W"], c["bias"], x)["dW"][:, 0]
        terms = (block[0] * (D * x).sum(0)).abs()
        assert float((dW - null).abs().max()) <= 1e-9 * float(terms.max())
        assert float(dW.abs().max()) <= 0.2 * float(terms.max())
