"""CPU: the Lovasz-Softmax rule (tests/lovasz_ref.py) against the authors' cumulative-sum formulation in fp64 torch autograd, the
facts the GPU tests rest on, the rule's mutants, the ABI, and the conditions the GPU cases rely on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lovasz_ref as L
from conftest import ROOT
from pointnet12_amd import _lib


def _tile():
    return int(_lib.load().pn2_lovasz_tile_rows())


def _random_segment(rng, n, ties=True):
    e = rng.random(n).astype(np.float32)
    if ties:
        e = np.where(rng.random(n) < 0.5, (rng.integers(0, 9, n) / 8.0).astype(np.float32), e)
    return e, rng.random(n) < rng.random()


def _authors_fp64(p, target, classes, images):
    """loss and d loss / d p of the authors' formulation in fp64 autograd: per image lovasz_softmax_flat on the kept rows, the mean
    over all images."""
    pt = torch.tensor(p.astype(np.float64), requires_grad=True)
    t = torch.tensor(target)
    N = p.shape[0] // images
    total = 0.0
    for b in range(images):
        keep = (t[b * N:(b + 1) * N] != L.IGNORE).nonzero().flatten() + b * N
        total = total + L.authors_flat_torch(pt[keep], t[keep], classes)
    loss = total / images
    if not torch.is_tensor(loss) or not loss.requires_grad:
        return float(loss), np.zeros(p.shape)
    loss.backward()
    return float(loss.detach()), pt.grad.numpy()


@pytest.mark.parametrize("classes,images", [("present", 1), ("all", 1), ([0, 2], 1), ("present", 3), ("all", 3)])
def test_rule_matches_the_authors_formulation_in_fp64_on_tie_free_inputs(classes, images):
    rng = np.random.default_rng(3)
    for trial in range(12):
        R, C = images * int(rng.integers(1, 120)), int(rng.integers(1, 6)) if classes != [0, 2] else 4
        p = (rng.integers(1, 2 ** 24, (R, C)) / 2.0 ** 24).astype(np.float32)      # multiples of 2^-24: 1 - p is exact in float32,
        t = L._random_target(rng, R, C, 0.2)                                       # so the rule's float32 error is the fp64 one
        e = np.abs(p - (t[:, None] == np.arange(C)[None]).astype(np.float32))
        assert all(np.unique(e[:, c]).size == R for c in range(C)), "tie-free"
        if images == 3 and trial % 2:
            t[R // 3:2 * (R // 3)] = L.IGNORE
        loss, dp = L.lovasz_rule(p, t, classes, images, L.IGNORE)
        want, grad = _authors_fp64(p, t, classes, images)
        assert abs(loss - want) <= 1e-12, (trial, loss, want)
        assert np.abs(dp - grad).max() <= 1e-12, trial


def test_closed_form_equals_the_cumulative_sum_form_bit_for_bit():
    rng = np.random.default_rng(0)
    for trial in range(2000):
        n = int(rng.integers(1, 200))
        e, fg = _random_segment(rng, n)
        order, ck, G = L.segment_terms(e, fg)
        gt = fg[order].astype(np.float64)
        gts = gt.sum()
        with np.errstate(invalid="ignore", divide="ignore"):
            jac = 1.0 - (gts - np.cumsum(gt)) / (gts + np.cumsum(1.0 - gt))
        jac[1:] = jac[1:] - jac[:-1]
        assert (jac.view(np.uint64) == ck.view(np.uint64)).all(), trial
        assert (ck >= 0).all() and ck.sum() <= 1.0, trial


def _seg_loss(e, fg, mutant=None):
    order, ck, _ = L.segment_terms(e, fg, mutant)
    return float(np.sum(e[order].astype(np.float64) * ck))


def test_value_ignores_tie_order_and_trailing_zero_rows_and_is_lipschitz():
    rng = np.random.default_rng(1)
    for trial in range(2000):
        n = int(rng.integers(1, 150))
        e, fg = _random_segment(rng, n)
        l = _seg_loss(e, fg)
        assert abs(l - _seg_loss(e, fg, "ties_desc_row")) <= 1e-13, trial       # the order among equal errors moves dp only
        m = int(rng.integers(1, 40))
        e2, fg2 = np.concatenate([e, np.zeros(m, np.float32)]), np.concatenate([fg, np.zeros(m, bool)])
        assert abs(l - _seg_loss(e2, fg2)) <= 1e-13, trial
        order, ck, _ = L.segment_terms(e, fg)
        order2, ck2, _ = L.segment_terms(e2, fg2)
        keep = order2 < n
        assert (order2[keep] == order).all() and np.abs(ck2[keep] - ck).max() <= 0.0 and (ck2[~keep][e2[order2][~keep] == 0] >= 0).all()
        e3 = np.clip(e + (rng.random(n).astype(np.float32) - 0.5) * np.float32(rng.random() * 0.2), 0, None).astype(np.float32)
        assert abs(l - _seg_loss(e3, fg)) <= np.abs(e3.astype(np.float64) - e).max() + 1e-13, trial


def _check_fails(case, loss, dp):
    want_loss, want_dp = L.rule_for(case)
    with np.errstate(over="ignore"):
        got_loss, got_dp = np.float32(loss), dp.astype(np.float32)
    return not (L.loss_close(got_loss, want_loss) and L.dp_equal(got_dp, want_dp))


def test_every_mutant_fails_a_check_on_every_case_it_changes():
    """What the GPU test asserts of the kernels (dp bit-equal in float32, loss the nearest float32 or its neighbour) tells the rule
    from each mutant on every case whose result the mutant changes, and each mutant changes some case."""
    cases = [c for c in L.exact_cases(_tile()) if c["p"].size <= 150000]
    changed = {m: 0 for m in L.MUTANTS}
    for case in cases:
        want_loss, want_dp = L.rule_for(case)
        for m in L.MUTANTS:
            loss, dp = L.lovasz_rule(case["p"], case["target"], case["classes"], case["images"], L.IGNORE, mutant=m)
            # "changes": beyond fp64 rounding (1e-12 relative and absolute).  Where a mutant only reorders rows of equal c_k, or
            # every row is foreground (c_k = 1 / G whatever the order), it adds the same terms in another order: no change
            with np.errstate(invalid="ignore"):
                same = bool(np.isclose(loss, want_loss, rtol=1e-12, atol=1e-12, equal_nan=True)) and \
                    bool(np.isclose(dp, want_dp, rtol=1e-12, atol=1e-12, equal_nan=True).all())
            if not same:
                changed[m] += 1
                assert _check_fails(case, loss, dp), (case["name"], m)
    assert all(n > 0 for n in changed.values()), changed


def test_abi_presence_and_version():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "pn2.h")).read()
    for name, nargs in (("pn2_lovasz_tile_rows", 0), ("pn2_lovasz_workspace_bytes", 3), ("pn2_lovasz_fwd", 16), ("pn2_lovasz_bwd", 10)):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, text), name
        assert len(_lib.SIGNATURES[name][1]) == nargs
    assert lib.pn2_version() == 15 == _lib.ABI_VERSION
    T = lib.pn2_lovasz_tile_rows()
    assert T >= 64 and T % 64 == 0
    # two key and two payload buffers dominate the workspace: 16 bytes per (row, class)
    for R, C, images in ((16 * 8000, 19, 16), (16 * 50000, 19, 16), (65536, 13, 1)):
        n = lib.pn2_lovasz_workspace_bytes(R, C, images)
        assert 16 * R * C <= n <= 16 * R * C * 1.2 + 65536, (R, C, n)
    assert lib.pn2_lovasz_workspace_bytes(10, 65, 1) == -1 and lib.pn2_lovasz_workspace_bytes(10, 3, 3) == -1
    assert lib.pn2_lovasz_workspace_bytes(0, 3, 1) == -1


def test_refusals_need_no_gpu():
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    assert lib.pn2_lovasz_fwd(one, 65, 0, one, 4, 65, 1, -100, 0, None, 1, one, one, None, one, None) == -1       # C > 64
    assert lib.pn2_lovasz_fwd(one, 2, 0, one, 4, 3, 1, -100, 0, None, 1, one, one, None, one, None) == -1         # pitch below C
    assert lib.pn2_lovasz_fwd(one, 3, 0, one, 4, 3, 3, -100, 0, None, 1, one, one, None, one, None) == -1         # images do not divide R
    assert lib.pn2_lovasz_fwd(one, 3, 0, one, 4, 3, 1, -100, 0, None, 1, None, one, None, one, None) == -1        # no workspace
    assert lib.pn2_lovasz_bwd(one, 3, 0, one, 4, 65, 1, one, one, None) == -1
    from pointnet12_amd.loss import LovaszSoftmax, lovasz_softmax
    assert LovaszSoftmax(classes="all", per_image=True).per_image
    with pytest.raises(TypeError):
        lovasz_softmax(torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(_lib.Pn2Error):
        lovasz_softmax(torch.zeros(4, 65), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(_lib.Pn2Error):
        lovasz_softmax(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64), per_image=True)
    with pytest.raises(_lib.Pn2Error):
        lovasz_softmax(torch.zeros(2, 3, 4, 5).permute(0, 1, 3, 2), torch.zeros(2, 5, 4, dtype=torch.int64))      # unsupported layout
    with pytest.raises(ValueError):
        lovasz_softmax(torch.zeros(0, 3), torch.zeros(0, dtype=torch.int64))
    with pytest.raises(_lib.Pn2Error):
        lovasz_softmax(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64))                                     # not on the GPU


def test_gpu_cases_hold_what_they_rely_on():
    T = _tile()
    cases = {c["name"]: c for c in L.exact_cases(T)}
    assert len(cases) == len(L.exact_cases(T)), "names are unique"
    for R in (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1):
        for C in (1, 2, 19, 64):
            c = cases["shape_R%d_C%d" % (R, C)]
            assert c["p"].shape == (R, C)
    assert all("shape_R%d_C%d" % (64 * T + 1, C) in cases for C in (1, 2, 19))
    big = cases["shape_R%d_C19" % (64 * T + 1)]
    assert big["p"].shape[0] > 64 * T                                     # more than 64 tiles per segment: a second scan step
    # ties are there: stability is exercised by the random cases too
    c = cases["shape_R%d_C19" % (T + 1)]
    assert np.unique(c["p"][:, 0]).size < c["p"].shape[0]
    c = cases["all_equal"]
    e = np.abs(c["p"] - (c["target"][:, None] == np.arange(3)[None]).astype(np.float32))
    assert (e == 0.5).all() and c["p"].shape[0] > 2 * T
    for name, sign in (("sorted", -1), ("reverse_sorted", 1)):
        c = cases[name]
        e0, e1 = c["p"][:, 0], np.abs(1 - c["p"][:, 1])
        assert (np.diff(e0) * sign >= 0).all() and (np.diff(e1) * sign >= 0).all() and np.unique(e0).size > T // 2
    c = cases["digit_pairs"]
    assert (L.key_of(c["p"][:, 0]) == c["digit_keys"]).all() and np.isfinite(c["p"]).all()
    for d, (lo, hi) in enumerate(L.digit_pair_keys()):
        assert lo ^ hi == (0xFF if d < 3 else 0x7F) << (8 * d) and (lo >> (8 * d)) & 0xFF == 0
        assert lo in c["digit_keys"] and hi in c["digit_keys"]
    k = c["digit_keys"].astype(np.int64)
    assert (k[0::2] > k[1::2]).all()                                      # the larger key first: each pair has to swap
    c = cases["zero_and_one"]
    e = np.abs(c["p"] - (c["target"][:, None] == np.arange(2)[None]))
    assert set(np.unique(e)) == {0.0, 1.0}
    c = cases["beyond_one"]
    assert np.isinf(c["p"]).any() and (c["p"] > 1).any() and (c["p"] < 0).any() and not np.isnan(c["p"]).any()
    c = cases["with_nan"]
    assert np.unique(c["p"][np.isnan(c["p"])].view(np.uint32)).size == 2  # two payloads, one key
    assert np.isnan(L.rule_for(c)[0])
    for name in ("first", "last", "interleaved"):
        t = cases["ignored_%s_present" % name]["target"]
        assert 0 < (t == L.IGNORE).sum() < t.size
    assert (cases["ignored_first_present"]["target"][:70] == L.IGNORE).all()
    assert (cases["ignored_last_present"]["target"][-70:] == L.IGNORE).all()
    for classes in ("present", "all"):
        c = cases["ignored_all_%s" % classes]
        loss, dp = L.rule_for(c)
        assert (c["target"] == L.IGNORE).all() and loss == 0.0 and not np.signbit(loss) and not dp.any()
    c = cases["out_of_range"]
    loss, dp = L.rule_for(c)
    assert np.isnan(loss) and not dp[list(c["bad_rows"])].any() and dp.any()
    assert all(c["target"][r] != L.IGNORE and not 0 <= c["target"][r] < 3 for r in c["bad_rows"])
    for name in ("present", "all", "list"):
        c = cases["absent_class_%s" % name]
        assert not (c["target"] == c["absent"]).any()
        dp = L.rule_for(c)[1]
        assert dp[:, 2].any() == (name != "present") and dp[:, 3].any() == (name != "list")
    c = cases["all_foreground"]
    assert (c["target"] == 1).all()
    for classes in ("present", "all"):
        c = cases["per_image_%s" % classes]
        N = c["p"].shape[0] // 3
        assert c["images"] == 3 and (c["target"][N:2 * N] == L.IGNORE).all() and N > T
        loss, dp = L.rule_for(c)
        assert not dp[N:2 * N].any() and dp[:N].any() and dp[2 * N:].any() and loss > 0
    for c in L.softmax_cases():
        assert c["x"].shape[0] <= 300 and c["x"].shape[0] % c["images"] == 0
