"""The Lovasz-Softmax rule of include/pn2.h (pn2_lovasz_fwd) in numpy, the authors' cumulative-sum formulation in torch, the rule's
mutants, and the table of cases the GPU tests run (tests/test_lovasz_cpu.py checks on the CPU what those cases rely on).

Berman, Triki, Blaschko, "The Lovasz-Softmax loss", CVPR 2018.  THE RULE AND ``authors_flat_torch`` ARE WRITTEN FROM THE PAPER AND FROM
MEMORY OF THE AUTHORS' PUBLISHED lovasz_softmax_flat / lovasz_grad AND ARE UNVERIFIED AGAINST THAT CODE, which was not available where
this was written."""
import numpy as np

MUTANTS = ("exclusive_F", "ascending", "ties_desc_row", "ignored_in_union", "absent_counted", "drop_low_digit",
           "per_image_nonempty", "sgn0_is_1")


def segment_order(e32, mutant=None):
    """Rule 3 and 4: rows by error descending, NaN first, equal errors in ascending row number."""
    n = e32.shape[0]
    e = e32
    if mutant == "drop_low_digit":
        e = (e32.view(np.uint32) & np.uint32(0xFFFFFF00)).view(np.float32)
    nan = np.isnan(e)
    sec = np.where(nan, 0.0, -e.astype(np.float64))
    if mutant == "ascending":
        sec = -sec
    tie = np.arange(n)
    if mutant == "ties_desc_row":
        tie = -tie
    return np.lexsort((tie, sec, ~nan))


def closed_form(k, F, G):
    """Rule 5: c_k in fp64 from integers (k 1-based rank, F_k foreground rows among the first k, G the foreground count)."""
    k, F = np.asarray(k, np.int64), np.asarray(F, np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        J = 1.0 - (G - F).astype(np.float64) / (G + k - F).astype(np.float64)
    Jp = np.concatenate([[0.0], J])[:-1]
    return J - Jp


def segment_terms(e32, fg, mutant=None):
    """-> (order, c_k along the order, G)."""
    order = segment_order(e32, mutant)
    fgs = fg[order].astype(np.int64)
    F = np.cumsum(fgs)
    G = int(F[-1]) if F.size else 0
    if mutant == "exclusive_F":
        F = F - fgs
    return order, closed_form(np.arange(1, e32.shape[0] + 1), F, G), G


def lovasz_rule(p, target, classes="present", images=1, ignore_index=-100, mutant=None):
    """p float32 [R, C] (the probabilities), target int64 [R] -> (loss fp64, dp fp64 [R, C]); float32 of either is what the kernels
    must return.  classes: "present", "all" or a list of ids; images: 1, or B for per_image."""
    p = np.ascontiguousarray(p, np.float32)
    target = np.asarray(target, np.int64)
    R, C = p.shape
    N = R // images
    part = (target != ignore_index) & (target >= 0) & (target < C)
    bad = bool((~part & (target != ignore_index)).any())
    if mutant == "ignored_in_union":
        part = part | (target == ignore_index)
    dp = np.zeros((R, C), np.float64)
    per_image = []
    for b in range(images):
        rows = np.arange(b * N, (b + 1) * N)[part[b * N:(b + 1) * N]]
        t, losses, segs = target[rows], [], []
        for c in range(C):
            fg = t == c
            if classes == "present":
                counted = bool(fg.any()) or mutant == "absent_counted"
            elif classes == "all":
                counted = True
            else:
                counted = c in classes
            if not counted:
                continue
            pc = p[rows, c]
            d = pc - fg.astype(np.float32)                                  # float32
            e = np.abs(d)                                                   # = fl32(|fg - p|)
            order, ck, _ = segment_terms(e, fg, mutant)
            with np.errstate(invalid="ignore"):
                losses.append(float(np.sum(e[order].astype(np.float64) * ck)))
            sg = (d > 0).astype(np.float64) - (d < 0).astype(np.float64)
            if mutant == "sgn0_is_1":
                sg = np.where(d == 0, 1.0, sg)
            cr = np.empty(rows.shape[0], np.float64)
            cr[order] = ck
            segs.append((c, cr, sg))
        per_image.append((rows, losses, segs))
    denom = images
    if mutant == "per_image_nonempty":
        denom = max(1, sum(1 for _, losses, _ in per_image if losses))
    total = 0.0
    for rows, losses, segs in per_image:
        if not losses:
            continue
        total += sum(losses) / float(len(losses))
        w = 1.0 / (float(len(losses)) * float(denom))
        for c, cr, sg in segs:
            dp[rows, c] = (w * cr) * sg
    loss = total / float(denom)
    return (float("nan") if bad else loss), dp


def authors_flat_torch(probas, labels, classes="present"):
    """The authors' lovasz_softmax_flat on [P, C] probabilities and [P] labels (ignored rows already removed), in torch."""
    import torch

    def lovasz_grad(gt_sorted):
        gts = gt_sorted.sum()
        intersection = gts - gt_sorted.cumsum(0)
        union = gts + (1.0 - gt_sorted).cumsum(0)
        jaccard = 1.0 - intersection / union
        if gt_sorted.shape[0] > 1:
            jaccard[1:] = jaccard[1:] - jaccard[:-1]
        return jaccard

    if probas.numel() == 0:
        return probas.sum() * 0.0
    C = probas.shape[1]
    losses = []
    for c in (list(range(C)) if classes in ("all", "present") else classes):
        fg = (labels == c).to(probas.dtype)
        if classes == "present" and fg.sum() == 0:
            continue
        errors = (fg - probas[:, c]).abs()
        errors_sorted, perm = torch.sort(errors, 0, descending=True)
        losses.append(torch.dot(errors_sorted, lovasz_grad(fg[perm])))
    if not losses:
        return probas.sum() * 0.0
    return sum(losses) / len(losses)


def key_of(e32):
    """The 32-bit sort key of an error (ascending key = descending error, every NaN first)."""
    e32 = np.asarray(e32, np.float32)
    bits = np.abs(e32).view(np.uint32).astype(np.int64)
    return np.where(np.isnan(e32), 0, 0x7FFFFFFF - bits).astype(np.uint32)


def error_of_key(key):
    return (np.uint32(0x7FFFFFFF) - np.asarray(key, np.uint32)).view(np.float32)


# ------------------------------------------------------------------------------------------------------------------ the cases
IGNORE = -100
DIGIT_BASE = 0x40A5C3E1          # digit pairs: this key with one digit forced to 0x00 and to 0xFF (the top one: 0x00 and 0x7F)


def digit_pair_keys():
    keys = []
    for d in range(4):
        lo = DIGIT_BASE & ~(0xFF << (8 * d)) & 0xFFFFFFFF
        hi = lo | ((0xFF if d < 3 else 0x7F) << (8 * d))
        keys.append((lo, hi))
    return keys


def _random_probs(rng, R, C):
    """float32 probabilities with many exact ties: half of the entries come from a grid of 17 values."""
    p = rng.random((R, C)).astype(np.float32)
    grid = (rng.integers(0, 17, (R, C)) / 16.0).astype(np.float32)
    return np.where(rng.random((R, C)) < 0.5, grid, p)


def _random_target(rng, R, C, ignored=0.1):
    t = rng.integers(0, C, R).astype(np.int64)
    t[rng.random(R) < ignored] = IGNORE
    return t


def _case(name, p, target, classes="present", images=1, **kw):
    return dict(name=name, p=np.ascontiguousarray(p, np.float32), target=np.asarray(target, np.int64), classes=classes, images=images, **kw)


def exact_cases(T):
    """The exact part's cases (from_logits=False) for a tile of T rows: name, p [R, C] float32, target, classes, images."""
    cases = []
    sizes = [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]
    for R in sizes:
        for C in (1, 2, 19, 64):
            rng = np.random.default_rng(1000 * C + R)
            cases.append(_case("shape_R%d_C%d" % (R, C), _random_probs(rng, R, C), _random_target(rng, R, C)))
    for C in (1, 2, 19):                                     # the second step of the per-segment tile scan
        R = 64 * T + 1
        rng = np.random.default_rng(7000 + C)
        cases.append(_case("shape_R%d_C%d" % (R, C), _random_probs(rng, R, C), _random_target(rng, R, C)))
    rng = np.random.default_rng(11)
    R = 2 * T + 1
    cases.append(_case("all_equal", np.full((R, 3), 0.5, np.float32), _random_target(rng, R, 3, 0.0)))
    R = T + 1
    ramp = np.linspace(0.0, 1.0, R, dtype=np.float32)
    # every row is class 1: class 0's error is p[:, 0] itself, class 1's is 1 - p[:, 1]
    cases.append(_case("sorted", np.stack([ramp[::-1], ramp], 1), np.ones(R, np.int64), classes="all"))
    cases.append(_case("reverse_sorted", np.stack([ramp, ramp[::-1]], 1), np.ones(R, np.int64), classes="all"))
    # pairs of keys that differ in one digit only, the larger key (smaller error) first: every pass has to move them
    rows = []
    for lo, hi in digit_pair_keys():
        rows += [hi, lo, hi, lo]
    e = error_of_key(np.array(rows * 40, np.uint32))
    cases.append(_case("digit_pairs", np.stack([e, np.full(e.shape, 0.5, np.float32)], 1), np.ones(e.shape[0], np.int64), classes="all",
                       digit_keys=np.array(rows * 40, np.uint32)))
    R = 300
    z = rng.integers(0, 2, (R, 2)).astype(np.float32)
    cases.append(_case("zero_and_one", z, _random_target(rng, R, 2)))
    R = T + 3
    big = _random_probs(rng, R, 3)
    big[::7, 0] = 2.5
    big[3::11, 1] = np.inf
    big[5::13, 2] = -0.5
    big[6::17, 0] = 3.0e38
    cases.append(_case("beyond_one", big, _random_target(rng, R, 3)))
    nan = big.copy()
    nan[2::9, 1] = np.nan
    nan[4::19, 1] = np.array([0x7FC01234], np.uint32).view(np.float32)[0]                  # another NaN payload: the same key
    cases.append(_case("with_nan", nan, _random_target(rng, R, 3)))
    R = T + 1
    for name, sel in (("first", np.arange(R) < 70), ("last", np.arange(R) >= R - 70), ("interleaved", np.arange(R) % 2 == 0),
                      ("all", np.ones(R, bool))):
        t = _random_target(rng, R, 3, 0.0)
        t[sel] = IGNORE
        for classes in (("present", "all") if name == "all" else ("present",)):
            cases.append(_case("ignored_%s_%s" % (name, classes), _random_probs(rng, R, 3), t, classes=classes))
    t = _random_target(rng, 200, 3)
    t[17], t[99] = 3, -1
    cases.append(_case("out_of_range", _random_probs(rng, 200, 3), t, bad_rows=(17, 99)))
    t = _random_target(rng, 500, 4)
    t[t == 2] = 1
    for classes in ("present", "all", [0, 2]):
        cases.append(_case("absent_class_%s" % (classes if isinstance(classes, str) else "list"), _random_probs(rng, 500, 4), t,
                           classes=classes, absent=2))
    cases.append(_case("all_foreground", _random_probs(rng, T + 1, 3), np.ones(T + 1, np.int64)))
    N = T + 1
    t = _random_target(rng, 3 * N, 3)
    t[N:2 * N] = IGNORE                                      # the middle image has no present class
    for classes in ("present", "all"):
        cases.append(_case("per_image_%s" % classes, _random_probs(rng, 3 * N, 3), t, classes=classes, images=3, empty_image=1))
    return cases


def softmax_cases():
    """from_logits=True: name, logits [R, C] float32, target, classes, images (R <= 300)."""
    cases = []
    for R in (1, 65, 300):
        for C in (2, 19, 64):
            rng = np.random.default_rng(50 * C + R)
            x = (3.0 * rng.standard_normal((R, C))).astype(np.float32)
            cases.append(dict(name="softmax_R%d_C%d" % (R, C), x=x, target=_random_target(rng, R, C), classes="present", images=1))
    rng = np.random.default_rng(5)
    x = (3.0 * rng.standard_normal((300, 13))).astype(np.float32)
    lp = (x.astype(np.float64) - np.log(np.exp(x.astype(np.float64)).sum(1, keepdims=True))).astype(np.float32)
    cases.append(dict(name="log_probabilities", x=lp, target=_random_target(rng, 300, 13), classes="present", images=1))
    cases.append(dict(name="softmax_per_image", x=x, target=_random_target(rng, 300, 13), classes="all", images=3))
    return cases


def softmax64(x):
    x = x.astype(np.float64)
    z = np.exp(x - x.max(1, keepdims=True))
    return z / z.sum(1, keepdims=True)


def loss_close(got32, want64):
    """got (float32) is the float32 nearest want (fp64) or its neighbour; NaN matches NaN, an infinity itself."""
    got32 = np.float32(got32)
    if np.isnan(want64):
        return bool(np.isnan(got32))
    with np.errstate(over="ignore"):
        near = np.float32(want64)
    if np.isinf(near) or near == got32:
        return bool(near == got32 or np.nextafter(near, np.float32(0)) == got32)
    return bool(np.nextafter(near, np.float32(np.inf)) == got32 or np.nextafter(near, np.float32(-np.inf)) == got32)


def dp_equal(got32, want64):
    """bit-equal float32 (a NaN matches a NaN)."""
    with np.errstate(over="ignore"):
        want = np.asarray(want64).astype(np.float32)
    got = np.asarray(got32, np.float32)
    return bool(((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all())


_rule_cache = {}


def rule_for(case):
    """The rule on an exact case, computed once per process."""
    if case["name"] not in _rule_cache:
        _rule_cache[case["name"]] = lovasz_rule(case["p"], case["target"], case["classes"], case["images"], IGNORE)
    return _rule_cache[case["name"]]
