"""CPU: the fp64 statement of the Adam rule and its error bound (tests/adam_ref.py), which tests/test_adam_abi_gpu.py holds
pn2_adam_step to.  Three jobs: (1) the fp32 oracle ``oracle/train_ref.adam_step`` lies within 2 E of it on every hyper-parameter set
and operand family; (2) wrong variants of the rule do not, so the acceptance has teeth; (3) ATen's own fp32 evaluation on the CPU
lies within the same 2 E.

Measured (200 000 elements per set): the oracle's worst |err| / (2 E) over p', m' and v' is 0.49 - 0.50 on every set (0.42 with
betas = (0, 0) and eps = 0, where m' = g exactly): it reaches the first-order bound and stays below the factor 2.  That needs the moments on the cancelling stride
g = -(fp32(wd) p) to be of that gradient's scale (adam_ref.make_inputs): with moments far below the rounding of wd p, m' and the
denominator are both nothing but rounding error, their quotient is a second-order term, and the ratio was seen at 0.89."""
import numpy as np
import pytest
import torch

import adam_ref as R
from oracle import train_ref as TR

N = 200000


def bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def oracle(p, g, m, v, hyper):
    """train_ref.adam_step on copies -> new (p', m', v')."""
    lr, betas, eps, wd, t = hyper
    p, m, v = p.copy(), m.copy(), v.copy()
    TR.adam_step(p, g.copy(), m, v, t, lr=lr, betas=betas, eps=eps, weight_decay=wd)
    return p, m, v


def violations(got, ref, E):
    """Per output the number of elements that are NOT within 2 E (a NaN is not)."""
    return [int((~(np.abs(a.astype(np.float64) - b) <= 2 * e)).sum()) for a, b, e in zip(got, ref, E)]


@pytest.fixture(scope="module")
def cases():
    out = []
    for k, hyper in enumerate(R.HYPER_SETS):
        p, g, m, v, plant = R.make_inputs(N, hyper, 100 + k)
        s = R.scalars(*hyper)
        ref, E = R.adam_ref(p, g, m, v, s)
        out.append((hyper, (p, g, m, v), plant, s, ref, E))
    return out


# ------------------------------------------------------------------------------------------------ 1. the oracle
def test_scalar_helper_forms_what_the_oracle_forms():
    """train_ref writes bc2 ** 0.5 where adam_scalars (and the helper) writes sqrt(bc2): the same fp32 number on every set, so the
    un-nudged candidate IS the oracle's.  A nudge moves exactly one ulp."""
    for lr, (b1, b2), eps, wd, t in R.HYPER_SETS:
        s = R.scalars(lr, (b1, b2), eps, wd, t)
        assert s.bc2_sqrt == float(np.float32((1 - b2 ** t) ** 0.5)) and s.step_size == float(np.float32(lr / (1 - b1 ** t)))
        assert s.beta1_w == float(np.float32(1 - b1)) and s.one_m_beta2 == float(np.float32(1 - b2))
        up, dn = R.scalars(lr, (b1, b2), eps, wd, t, (1, -1)), R.scalars(lr, (b1, b2), eps, wd, t, (-1, 1))
        assert dn.step_size < s.step_size < up.step_size or lr == 0
        assert up.bc2_sqrt < s.bc2_sqrt < dn.bc2_sqrt
        assert np.nextafter(np.float32(up.bc2_sqrt), np.float32(9)) == np.float32(s.bc2_sqrt)
        assert up[2:] == s[2:] == dn[2:]
    assert len(set(R.NUDGES)) == 9 and R.NUDGES[0] == (0, 0)


def test_oracle_within_the_bound_on_every_set_and_family(cases):
    print()
    for hyper, (p, g, m, v), plant, s, ref, E in cases:
        got = oracle(p, g, m, v, hyper)
        assert all(np.isfinite(x).all() for x in got)
        ratios = [R.worst_ratio(a, b, e) for a, b, e in zip(got, ref, E)]
        print("adam oracle vs fp64, %-40s worst |err|/(2E): p %.3f  m %.3f  v %.3f" % (hyper, *ratios))
        assert max(ratios) <= 1.0, (hyper, ratios)
        # the statement on given scalars is the oracle, bit for bit
        for a, b, what in zip(R.adam_f32(p, g, m, v, s), got, "pmv"):
            assert (bits(a) == bits(b)).all(), (hyper, what)
        # the planted group (g = m = v = 0, eps > 0) keeps the bits of p
        assert plant.size or hyper[2] == 0
        assert (bits(got[0])[plant] == bits(p)[plant]).all() and not got[1][plant].any() and not got[2][plant].any()
        if hyper[0] == 0:
            # lr = 0: p - 0 * x keeps p, but for -0 - (-0) = +0 (IEEE, ATen does the same): equal values, and equal bits off -0
            assert (got[0] == p).all() and (bits(got[0]) == bits(p))[bits(p) != 0x80000000].all()
            assert (bits(got[1]) != bits(m)).any() and (bits(got[2]) != bits(v)).any()


def test_the_families_are_what_they_claim(cases):
    for hyper, (p, g, m, v), plant, s, ref, E in cases:
        lr, betas, eps, wd, t = hyper
        assert (bits(p) == 0).any() and (bits(p) == 0x80000000).any() and (np.abs(p) >= 1e4).any()
        nz = g != 0
        assert np.abs(g[nz]).min() >= np.float32(1e-12) and np.abs(g).max() > 100 and (np.abs(g[nz]) < 1e-10).any()
        assert (not nz[::7].any()) if eps != 0 else nz.all()
        if wd != 0:
            c = R.cancel_mask(N)
            assert (g[c] + np.float32(wd) * p[c] == 0).all() and (g[c] != 0).any()
        assert (t == 1) == (not m.any() and not v.any())
        # no intermediate is denormal: the smallest are (1 - beta2) g^2 and beta2 v
        tiny = np.finfo(np.float32).tiny
        assert (1 - betas[1]) * float(np.abs(g[nz]).min()) ** 2 > tiny and (t == 1 or betas[1] * float(v[v != 0].min()) > tiny)


# ------------------------------------------------------------------------------------------------ 2. wrong variants
def test_wrong_variants_violate_the_bound(cases):
    """eps dropped, wd dropped, bc2_sqrt replaced by 1 (at t = 7), beta2 and 1 - beta2 swapped: each on the inputs the oracle passes
    on, on every set where the variant changes the rule, breaks 2 E on FINITE elements (dropping eps also turns 0/0 into NaN where
    g = 0; those are not counted here)."""
    print()
    hit = {"eps": 0, "wd": 0, "bc2": 0, "swap": 0}
    for hyper, (p, g, m, v), plant, s, ref, E in cases:
        lr, betas, eps, wd, t = hyper
        variants = {}
        if eps != 0 and lr != 0:
            variants["eps"] = s._replace(eps=0.0)
        if wd != 0:
            variants["wd"] = s._replace(wd=0.0)
        if t == 7:
            variants["bc2"] = s._replace(bc2_sqrt=1.0)
        if betas[1] != 0.5:
            variants["swap"] = s._replace(beta2=s.one_m_beta2, one_m_beta2=s.beta2)
        for name, sv in variants.items():
            got = R.adam_f32(p, g, m, v, sv)
            fin = [np.isfinite(x) for x in got]
            bad = violations(*([x[f] for x, f in zip(xs, fin)] for xs in (got, ref, E)))
            print("adam variant %-4s %-40s elements outside 2E: p %d  m %d  v %d" % (name, hyper, *bad))
            assert sum(bad) > 0, (name, hyper)
            hit[name] += 1
    assert all(hit.values()), hit


def test_wrong_lerp_form_is_caught():
    """ATen's lerp has two forms of one function, m + w d for w < 0.5 and g - d (1 - w) otherwise.  Taking the other form is caught
    * at beta1 = 0.9 (w = 0.1, the high form forced) by the bound: |err| reaches 3 x 2 E on m';
    * at beta1 = 0.3 (w = 0.7, the low form forced) NOT by the bound, and it cannot be.  The two forms differ by their roundings
      alone.  The low form's are w ulp(d)/2 + ulp(w d)/2 (+ the last add, which both have), the bound of the right form is
      2 (1 - w) 2^-24 |d|, twice that 1.2 * 2^-24 |d|.  With d = x 2^e, 1 <= x < 2: for x < 1/0.7 the low form's roundings are at most
      (0.7 + 0.5) 2^-24 2^e <= 1.2 x 2^-24 2^e, for x >= 1/0.7 at most 1.7 2^-24 2^e <= 1.2 x 2^-24 2^e.  Measured: 0.72 of 2 E.
      It IS caught by the other half of the acceptance, the bits of m': they differ from the oracle's on a third of the elements."""
    print()
    for k, min_ratio, min_differ in ((1, 2.0, N // 4), (3, None, N // 4)):
        hyper = R.HYPER_SETS[k]
        p, g, m, v, _ = R.make_inputs(N, hyper, 100 + k)
        s = R.scalars(*hyper)
        ref, E = R.adam_ref(p, g, m, v, s)
        good = oracle(p, g, m, v, hyper)
        got = R.adam_f32(p, g, m, v, s, low_form=not s.beta1_w < 0.5)
        ratio = R.worst_ratio(got[1], ref[1], E[1])
        differ = int((bits(got[1]) != bits(good[1])).sum())
        print("adam wrong lerp form at beta1 = %g: m' worst |err|/(2E) %.3f, bits differ from the oracle on %d of %d" % (
            hyper[1][0], ratio, differ, N))
        assert differ >= min_differ
        assert (bits(got[2]) == bits(good[2])).all()
        if min_ratio is not None:
            assert ratio > min_ratio
    # at w exactly 0.5 the boundary belongs to the high form: the low form differs in bits there too
    hyper = R.HYPER_SETS[4]
    p, g, m, v, _ = R.make_inputs(N, hyper, 104)
    s = R.scalars(*hyper)
    assert s.beta1_w == 0.5
    assert (bits(R.adam_f32(p, g, m, v, s, low_form=True)[1]) != bits(oracle(p, g, m, v, hyper)[1])).any()


# ------------------------------------------------------------------------------------------------ 3. ATen on the CPU
@pytest.mark.parametrize("k", range(len(R.HYPER_SETS)), ids=R.HYPER_IDS)
def test_aten_single_tensor_adam_within_the_bound(k):
    """torch.optim.Adam(foreach=False) on CPU tensors, two steps from zero state, each step held to adam_ref on the state ATen
    entered it with and the helper's scalars for that step.  ATen's vector kernels fuse some multiply-adds (fewer roundings than
    the rule counts), which the bound allows without widening any term."""
    lr, betas, eps, wd, _ = R.HYPER_SETS[k]
    n = 50000
    p0 = R.make_inputs(n, (lr, betas, eps, wd, 1), 200 + k)[0]
    param = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([param], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    print()
    for t in (1, 2):
        # the gradient family of step t on the parameters as they are now (the cancelling stride follows p)
        p = param.detach().numpy().copy()
        g = R.make_inputs(n, (lr, betas, eps, wd, t), 300 + 10 * k + t)[1]
        if wd != 0:
            c = R.cancel_mask(n)
            g[c] = -(np.float32(wd) * p[c])
        ref, E = R.adam_ref(p, g, m, v, R.scalars(lr, betas, eps, wd, t))
        param.grad = torch.from_numpy(g.copy())
        opt.step()
        st = opt.state[param]
        got = (param.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy())
        assert float(st["step"]) == t
        ratios = [R.worst_ratio(a, b, e) for a, b, e in zip(got, ref, E)]
        print("ATen CPU Adam vs fp64, %s step %d: worst |err|/(2E): p %.3f  m %.3f  v %.3f" % (R.HYPER_IDS[k], t, *ratios))
        assert max(ratios) <= 1.0, (t, ratios)
        m, v = got[1], got[2]
