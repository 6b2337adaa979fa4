"""numpy restatement of the segment-reduction rules (include/pn2.h, ``pn2_segment_mean`` / ``pn2_segment_mean_bwd`` /
``pn2_segment_mode``), for the tests.

The mean of a segment's column: a finite float32 is ``s * M * 2**(k - 150)`` (exponent field ``e >= 1``: ``M = 2**23 + fraction``,
``k = e``; ``e == 0``: ``M = fraction``, ``k = 1``); ``K`` is the column's largest ``k``; a term contributes the integer
``t = s * ((M << 10) >> (K - k))`` (0 when ``K - k >= 34``); ``S = sum(t)`` in int64, exact in any order;
``mean = float32(ldexp(float64(S) / float64(n), K - 160))``.  A NaN / inf term makes the column the quiet NaN ``0x7FC00000``; a
segment without rows gives ``+0.0``.  Everything below works on ONE cloud: ``seg`` holds ranks, a negative one takes no part.
"""
from fractions import Fraction

import numpy as np

QUIET_NAN = 0x7FC00000
ERR_RANGE, ERR_NONFINITE = 4, 8                                      # PN2_SEGMENT_ERR_* of include/pn2.h


def decompose(values):
    """``(sign int64 (+1 / -1), M int64, k int64, finite bool)`` of float32 ``values``, elementwise."""
    bits = np.ascontiguousarray(values, np.float32).view(np.uint32).astype(np.int64)
    e, frac = (bits >> 23) & 255, bits & 0x7FFFFF
    return np.where(bits >> 31 != 0, -1, 1), np.where(e == 0, frac, frac | (1 << 23)), np.where(e == 0, 1, e), e != 255


def takes_part(seg, count):
    """``(part bool [M], err)``: rows with ``0 <= seg < count`` take part; a ``seg >= count`` sets ``ERR_RANGE``."""
    seg = np.asarray(seg, np.int64)
    return (seg >= 0) & (seg < count), (ERR_RANGE if (seg >= count).any() else 0)


def segment_mean(values, seg, count, n=None):
    """``values`` float32 ``[M, C]``, ``seg`` int ``[M]`` -> a dict: ``mean`` float32 ``[count, C]`` (compare its BITS), ``n`` int32
    ``[count]`` (the rows that took part, or the given ``n``), ``K`` / ``S`` int64 ``[count, C]`` and ``err``."""
    values = np.ascontiguousarray(values, np.float32)
    M, C = values.shape
    part, err = takes_part(seg, count)
    rows = np.flatnonzero(part)
    s = np.asarray(seg, np.int64)[rows]
    sign, mant, k, finite = decompose(values[rows])
    K = np.zeros((count, C), np.int64)
    np.maximum.at(K, s, np.where(finite, k, 255))
    down = K[s] - k
    t = np.where((down >= 34) | (K[s] == 255), 0, sign * ((mant << 10) >> np.clip(down, 0, 62)))
    S = np.zeros((count, C), np.int64)
    np.add.at(S, s, t)                                               # integers: exact, whatever the order
    if n is None:
        n = np.bincount(s, minlength=count)
    n = np.asarray(n, np.int64)[:count]
    nn = np.maximum(n, 1)[:, None].astype(np.float64)
    with np.errstate(all="ignore"):
        mean = np.ldexp(S.astype(np.float64) / nn, (K - 160).astype(np.int32)).astype(np.float32)
    mean = np.where((n[:, None] <= 0) | (K == 0), np.float32(0.0), mean).astype(np.float32)
    out = mean.view(np.uint32).copy()
    out[K == 255] = QUIET_NAN
    if (K == 255).any():
        err |= ERR_NONFINITE
    return {"mean": out.view(np.float32), "n": n.astype(np.int32), "K": K, "S": S, "err": err}


def exact_mean(column):
    """The exact mean of a 1-D float32 array as a ``Fraction``."""
    return sum((Fraction(float(v)) for v in np.asarray(column, np.float32)), Fraction(0)) / len(column)


def ulp32(x):
    """The spacing of float32 at ``|x|`` (a ``Fraction``): 2**-149 in the subnormal range."""
    x = abs(Fraction(x))
    if x < Fraction(2) ** -126:
        return Fraction(2) ** -149
    e = 0
    while Fraction(2) ** (e + 1) <= x:                               # floor(log2 x), exactly
        e += 1
    while Fraction(2) ** e > x:
        e -= 1
    return Fraction(2) ** (e - 23)


def mean_bound(K, exact, mean):
    """The derived bound of include/pn2.h: ``2**(K - 160) + ulp32(mean) / 2 + |exact| * 2**-51`` (a ``Fraction``)."""
    return Fraction(2) ** (int(K) - 160) + ulp32(Fraction(float(mean))) / 2 + abs(exact) * Fraction(2) ** -51


def segment_mean_bwd(grad_out, seg, count, n):
    """``grad_in[row] = float32(grad_out[seg[row]]) / float32(n[seg[row]])``, ``+0.0`` for a row that takes no part."""
    grad_out = np.ascontiguousarray(grad_out, np.float32)
    part, err = takes_part(seg, count)
    s = np.where(part, np.asarray(seg, np.int64), 0)
    nf = np.asarray(n, np.int32)[s].astype(np.float32)[:, None]
    with np.errstate(all="ignore"):
        g = (grad_out[s] / np.where(nf > 0, nf, np.float32(1.0))).astype(np.float32)
    g[~part | (nf[:, 0] <= 0)] = 0.0
    return g, err


def segment_mode(labels, seg, count, fill=-1):
    """``(winner int32 [count], votes int32 [count], err)``: most votes, the LOWEST label among equals, ``fill`` without a voter."""
    labels = np.asarray(labels, np.int64)
    part, err = takes_part(seg, count)
    vote = part & (labels >= 0)
    winner, votes = np.full(count, fill, np.int32), np.zeros(count, np.int32)
    if vote.any():
        pair = (np.asarray(seg, np.int64)[vote] << 32) | labels[vote]
        uniq, cnt = np.unique(pair, return_counts=True)
        # by segment, then by count descending, then by label ascending: the first of every segment wins
        order = np.lexsort((uniq & 0xFFFFFFFF, -cnt, uniq >> 32))
        s_sorted = (uniq >> 32)[order]
        first = np.flatnonzero(np.r_[True, s_sorted[1:] != s_sorted[:-1]])
        winner[s_sorted[first]] = (uniq & 0xFFFFFFFF)[order][first].astype(np.int32)
        votes[s_sorted[first]] = cnt[order][first].astype(np.int32)
    return winner, votes, err
