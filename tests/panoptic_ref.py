"""The panoptic-quality rule of include/pn2.h ("panoptic quality") in numpy, written the way the SemanticKITTI API's ``PanopticEval``
writes it: per cloud, per class and per side one ``np.unique`` over the ids (0 = none after the API's ``+ 1``), one over the combined
ids for the intersections.  WRITTEN FROM MEMORY OF THE API AND UNVERIFIED AGAINST IT.  The table is exact (Python / int64 integers);
beside it the API-style fp64 running sum of the IoUs is kept, for the stated deviation bound.

``mutant=`` builds one deliberate mistake into the rule (tests/test_panoptic_cpu.py shows that each changes a table)."""
import numpy as np

ERR_CLASS, ERR_ROWS = 256, 512                                       # PN2_PANOPTIC_ERR_* of include/pn2.h
COLUMNS = ("tp", "fp", "fn", "iou_hi", "iou_lo")
EPS = 1e-15                                                          # the API's
MUTANTS = ("ge_half", "area_gt_min", "ignored_kept", "no_class_key", "no_cloud_key", "cross_class", "no_things")
ONE = 1 << 53


def iou_integer(inter, union):
    """``(q, t)``: the fp64 quotient (ONE division, the API's ``iou``) and the integer ``q * 2^53``; raises if that is no integer."""
    q = float(inter) / float(union)
    t = q * float(ONE)                                               # a power-of-two scaling: exact
    if t != int(t):
        raise AssertionError("q * 2^53 is no integer for %d / %d" % (inter, union))
    return q, int(t)


def _dense(cls, inst1, with_class):
    """Ids 1 .. K per distinct (class, id + 1) among the rows whose ``inst1`` is non-zero (0 elsewhere), and K."""
    has = inst1 > 0
    dense = np.zeros(len(inst1), np.int64)
    if not has.any():
        return dense, 0
    keys = ((cls[has] << 32) if with_class else 0) | inst1[has]     # (0 <= class < C, 0 < id + 1 <= 2^31: one int64 word)
    uniq, inverse = np.unique(keys, return_inverse=True)
    dense[has] = inverse.reshape(-1) + 1
    return dense, len(uniq)


def _cloud(ps, pi, gs, gi, C, include, things, min_points, mutant, table, fsum):
    """One cloud's rows added into ``table`` int64 [C, 5] and ``fsum`` fp64 [C]; returns the error bits."""
    ps, pi, gs, gi = (np.asarray(a, np.int64) for a in (ps, pi, gs, gi))
    in_range = (gs >= 0) & (gs < C)
    err = 0 if in_range.all() else ERR_CLASS
    keep = in_range & (include[np.clip(gs, 0, C - 1)] != 0)           # rule 1: every other row leaves BOTH sides
    pred_class = (ps >= 0) & (ps < C)
    pred_class &= include[np.clip(ps, 0, C - 1)] != 0
    if things is not None and mutant != "no_things":                 # a stuff class: one segment, id 0
        gi = np.where(in_range & (things[np.clip(gs, 0, C - 1)] == 0), 0, gi)
        pi = np.where(pred_class & (things[np.clip(ps, 0, C - 1)] == 0), 0, pi)
    g_rows = keep & (gi >= 0)
    p_rows = pred_class & (pi >= 0) & (keep | (mutant == "ignored_kept"))
    g1, p1 = np.where(g_rows, gi + 1, 0), np.where(p_rows, pi + 1, 0)    # the API's + 1: 0 means "no segment"
    with_class = mutant != "no_class_key"
    gd, n_g = _dense(gs, g1, with_class)
    pd, n_p = _dense(ps, p1, with_class)
    g_area, p_area = np.bincount(gd, minlength=n_g + 1), np.bincount(pd, minlength=n_p + 1)
    g_matched, p_matched = np.zeros(n_g + 1, bool), np.zeros(n_p + 1, bool)
    offset = 1 << 32
    classes = [c for c in range(C) if include[c] != 0]
    for cl in classes:
        g_inst, p_inst = gd * (gs == cl), pd * (ps == cl)
        if mutant == "cross_class":
            p_inst = pd
        valid = (g_inst > 0) & (p_inst > 0) & keep
        comb, inter = np.unique(g_inst[valid] * offset + p_inst[valid], return_counts=True)
        g_ids, p_ids = comb // offset, comb % offset
        union = g_area[g_ids] + p_area[p_ids] - inter
        match = 2 * inter >= union if mutant == "ge_half" else 2 * inter > union      # rule 9, on integers
        for k in np.flatnonzero(match):
            q, t = iou_integer(int(inter[k]), int(union[k]))
            table[cl, 0] += 1
            table[cl, 3] += t >> 32
            table[cl, 4] += t & 0xFFFFFFFF
            fsum[cl] += q                                            # the API: a running fp64 sum
        g_matched[g_ids[match]] = True
        p_matched[p_ids[match]] = True
    for cl in classes:
        g_here, p_here = np.unique(gd[(gd > 0) & (gs == cl)]), np.unique(pd[(pd > 0) & (ps == cl)])
        big = (lambda a: a > min_points) if mutant == "area_gt_min" else (lambda a: a >= min_points)
        table[cl, 2] += int((big(g_area[g_here]) & ~g_matched[g_here]).sum())
        table[cl, 1] += int((big(p_area[p_here]) & ~p_matched[p_here]).sum())
    return err


def panoptic_table(pred_sem, pred_inst, gt_sem, gt_inst, C, include=None, things=None, min_points=30, begins=None, counts=None,
                   max_rows=None, per_cloud=False, mutant=None):
    """``(table, fsum, err)``: int64 ``[C, 5]`` (``[B, C, 5]`` with ``per_cloud``), the API-style fp64 IoU sums in the same leading
    shape, the error bits.  Clouds: ``begins`` / ``counts`` (None: one cloud, every row), counts clamped to ``[0, max_rows]``; a cloud
    that leaves the arrays is skipped whole and sets ``ERR_ROWS``."""
    assert mutant is None or mutant in MUTANTS
    rows = len(gt_sem)
    include = np.ones(C, np.int64) if include is None else np.asarray(include, np.int64)
    things = None if things is None else np.asarray(things, np.int64)
    begins, counts = ([0], [rows]) if begins is None else (list(begins), list(counts))
    max_rows = rows if max_rows is None else max_rows
    B = len(begins)
    table, fsum, err = np.zeros((B if per_cloud else 1, C, 5), np.int64), np.zeros((B if per_cloud else 1, C)), 0
    spans = []
    for b in range(B):
        n = max(0, min(int(counts[b]), max_rows))
        if begins[b] < 0 or begins[b] > rows - n:
            err |= ERR_ROWS
            continue
        spans.append((b, np.arange(begins[b], begins[b] + n)))
    if mutant == "no_cloud_key" and spans:
        spans = [(0, np.concatenate([s for _, s in spans]))]
    for b, s in spans:
        at = b if per_cloud else 0
        err |= _cloud(np.asarray(pred_sem)[s], np.asarray(pred_inst)[s], np.asarray(gt_sem)[s], np.asarray(gt_inst)[s], C, include, things,
                      min_points, mutant, table[at], fsum[at])
    return (table, fsum, err) if per_cloud else (table[0], fsum[0], err)


def iou_sum(table):
    """Per class ``S / 2^53``, ``S = iou_hi * 2^32 + iou_lo`` as a Python integer: ONE correctly rounded division."""
    return np.array([((int(r[3]) << 32) + int(r[4])) / ONE for r in np.asarray(table).reshape(-1, 5)]).reshape(np.asarray(table).shape[:-1])


def deviation_bound(table):
    """|exact sum - running fp64 sum| <= n_tp * 2^-52 * sum, per class (include/pn2.h: the stated deviation)."""
    t = np.asarray(table)
    return t[..., 0] * 2.0 ** -52 * iou_sum(t)


def api_scores(table, fsum, include=None):
    """The API's ``getPQ`` on the counts and ITS fp64 IoU sum: dict of pq / sq / rq (means over the included classes) and per class."""
    t = np.asarray(table).astype(np.float64)
    C = t.shape[0]
    inc = np.ones(C, bool) if include is None else np.asarray(include) != 0
    tp, fp, fn = t[:, 0], t[:, 1], t[:, 2]
    sq = np.asarray(fsum, np.float64) / np.maximum(tp, EPS)
    rq = tp / np.maximum(tp + 0.5 * fp + 0.5 * fn, EPS)
    pq = sq * rq
    return {"pq": pq[inc].mean(), "sq": sq[inc].mean(), "rq": rq[inc].mean(), "pq_per_class": pq, "sq_per_class": sq, "rq_per_class": rq}


# ------------------------------------------------------------------------------------------------------------------ cases
def blocks(*spec):
    """``(n, pred_sem, pred_inst, gt_sem, gt_inst)`` blocks -> four int64 arrays of the blocks' rows, in order."""
    cols = [np.concatenate([np.full(b[0], b[k], np.int64) for b in spec]) if spec else np.zeros(0, np.int64) for k in range(1, 5)]
    return tuple(cols)


FULL = [1, 0, 0, 1 << 21, 0]                                         # one match of IoU 1: t = 2^53
Q_6_11 = [1, 0, 0, 0x11745D, 0x1745D174]                             # 6 / 11 in fp64 is 0x3FE1745D1745D174: the 53-bit integer 0x11745D1745D174
Q_2_3 = [1, 0, 0, 0x155555, 0x55555555]                              # 2 / 3 is 0x3FE5555555555555: 0x15555555555555
BIG = 2 ** 31 - 1


def hand_cases():
    """Small cases worked by hand: ``name -> dict`` of the call's arguments and the expected ``table`` (lists ``[C][5]``) and ``err``."""
    out = {}

    def case(name, rows, C, table, include=None, things=None, min_points=1, begins=None, counts=None, err=0):
        ps, pi, gs, gi = rows
        out[name] = {"pred_sem": ps, "pred_inst": pi, "gt_sem": gs, "gt_inst": gi, "C": C, "include": include, "things": things,
                     "min_points": min_points, "begins": begins, "counts": counts, "table": np.array(table, np.int64), "err": err}

    zero = [0, 0, 0, 0, 0]
    # the threshold: IoU 1/2 and 5/10 are no match (one fp, one fn), 6/11 is
    case("iou_1_2", blocks((1, 0, 1, 0, 1), (1, 0, 1, 0, -1)), 1, [[0, 1, 1, 0, 0]])
    case("iou_5_10", blocks((5, 0, 3, 0, 7), (5, 0, 3, 0, -1)), 1, [[0, 1, 1, 0, 0]])
    case("iou_6_11", blocks((6, 0, 3, 0, 7), (5, 0, 3, 0, -1)), 1, [Q_6_11])
    # unmatched segments of area min_points - 1 and min_points on each side (ground truth ids 1, 2; predicted ids 5, 6)
    sides = blocks((3, 0, -1, 0, 1), (4, 0, -1, 0, 2), (3, 0, 5, 0, -1), (4, 0, 6, 0, -1))
    case("min_points_4", sides, 1, [[0, 1, 1, 0, 0]], min_points=4)
    case("min_points_0", sides, 1, [[0, 2, 2, 0, 0]], min_points=0)
    case("min_points_1", sides, 1, [[0, 2, 2, 0, 0]], min_points=1)
    # one id under two classes: two segments per side, each matched whole (with the class left out of the key: areas 6, no match)
    case("id_under_two_classes", blocks((3, 0, 4, 0, 4), (3, 1, 4, 1, 4)), 2, [FULL, FULL])
    # one (class, id) in two clouds: two segments per side (pooled into one cloud it would be ONE match)
    case("key_in_two_clouds", blocks((3, 0, 1, 0, 1), (3, 0, 1, 0, 1)), 1, [[2, 0, 0, 2 << 21, 0]], begins=[0, 3], counts=[3, 3])
    # a stuff class whose ids differ row by row (a -1 among them): one segment per side, matched whole; class 1 is a thing
    ps, pi, gs, gi = blocks((6, 0, 0, 0, 0), (2, 1, 9, 1, 9))
    pi[:6], gi[:6] = [5, 6, 7, -1, 9, 10], [-1, 11, 12, 13, 14, BIG]
    case("things_mask", (ps, pi, gs, gi), 2, [FULL, FULL], things=[0, 1])
    # without the mask the rows 1, 2, 4, 5 are four one-row matches, row 0 one fp, row 3 one fn
    case("things_mask_absent", (ps, pi, gs, gi), 2, [[4, 1, 1, 4 << 21, 0], FULL])
    # ids -1 and 2^31 - 1 under class C - 1
    case("id_edges", blocks((4, 2, BIG, 2, BIG), (3, 2, -1, 2, -1), (2, 2, -1, 2, BIG)), 3, [zero, zero, Q_2_3])
    # a gt_sem outside [0, C): the error bit, the row leaves both sides (the predicted segment shrinks to the two rows that match)
    ps, pi, gs, gi = blocks((2, 0, 1, 0, 1), (4, 0, 1, 0, 1))
    gs[2:] = [-1, 2, BIG, -BIG - 1]
    case("class_out_of_range", (ps, pi, gs, gi), 2, [FULL, zero], err=ERR_CLASS)
    # dropping the ignored rows (class 2) lifts a predicted segment across 1/2: 4 of 9 rows become 4 of 4 ...
    case("ignored_rows_lift", blocks((4, 0, 1, 0, 1), (5, 0, 1, 2, 8)), 3, [FULL, zero, zero], include=[1, 1, 0])
    # ... and only AT it where four more rows are not ignored: 4 of 8, no match.  (An ignored row is in no ground-truth segment, so the
    # drop never lowers a pair's IoU; what it can take away is an fp: the predicted segment of class 1 falls from 4 rows to 1.)
    case("ignored_rows_stay", blocks((4, 0, 1, 0, 1), (4, 0, 1, 0, -1), (5, 0, 1, 2, 8), (1, 1, 3, 0, -1), (3, 1, 3, 2, 8)), 3,
         [[0, 1, 1, 0, 0], zero, zero], include=[1, 1, 0], min_points=2)
    # a pair across classes is no pair: one fn under the ground truth's class, one fp under the prediction's
    case("pair_across_classes", blocks((3, 1, 1, 0, 1)), 2, [[0, 0, 1, 0, 0], [0, 1, 0, 0, 0]])
    # a predicted class that is excluded, beyond C or negative: no predicted segment, the ground truth stays unmatched
    case("pred_class_unusable", blocks((2, 2, 1, 0, 1), (2, 7, 1, 0, 1), (2, -3, 1, 0, 1)), 3, [[0, 0, 1, 0, 0], zero, zero],
         include=[1, 1, 0])
    return out


def random_case(seed, n, C=5, segments=12, B=1, ignore_class=True, noise=0.15, things=True, ids=40):
    """A seeded scene of ``B`` clouds of ``n`` rows each, back to back: ground-truth segments as runs of rows, a prediction that
    follows them with shifted borders, relabelled rows, split and missing ids.  Ids are drawn below ``ids``: with few of them, runs far
    apart share a segment.  Returns the keyword arguments of ``panoptic_table``."""
    rng = np.random.default_rng(seed)
    ps, pi, gs, gi = (np.zeros(B * n, np.int64) for _ in range(4))
    for b in range(B):
        lo = b * n
        cuts = np.sort(rng.integers(0, n + 1, max(segments - 1, 0)))
        edges = np.concatenate([[0], cuts, [n]])
        for k in range(len(edges) - 1):
            a, e = lo + edges[k], lo + edges[k + 1]
            cls, ident = rng.integers(0, C), rng.integers(0, ids)
            gs[a:e], gi[a:e] = cls, ident
            shift = int(rng.integers(-3, 4)) if e - a > 8 else 0
            a2, e2 = max(lo, a + shift), min(lo + n, e + shift)
            ps[a2:e2], pi[a2:e2] = cls, ident + (100 if rng.random() < 0.2 else 0)
            if e - a > 6 and rng.random() < 0.3:                       # the prediction splits the segment near its middle or third
                pi[a + (e - a) // int(rng.integers(2, 4)):e2] = ident + 50
    flip = rng.random(B * n) < noise
    ps[flip] = rng.integers(-1, C + 1, int(flip.sum()))
    flip = rng.random(B * n) < noise
    pi[flip] = rng.integers(-1, ids, int(flip.sum()))
    gi[rng.random(B * n) < 0.03] = -1
    include = np.ones(C, np.int64)
    if ignore_class and C > 1:
        include[0] = 0
    th = None
    if things and C > 2:
        th = np.ones(C, np.int64)
        th[C - 1] = 0
    return {"pred_sem": ps, "pred_inst": pi, "gt_sem": gs, "gt_inst": gi, "C": C, "include": include, "things": th,
            "min_points": int(rng.integers(0, 6)), "begins": [b * n for b in range(B)], "counts": [n] * B}
