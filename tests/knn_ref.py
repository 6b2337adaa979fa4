"""fp64 statements of pn2_knn and pn2_knn_vote (include/pn2.h), written in numpy as plain loops, for clarity, not speed.
On the lattice inputs of tests/geometry_ref.py the float32 distance IS the fp64 distance, so a kernel must reproduce
``knn64`` index for index and bit for bit, and ``vote_ref`` -- integers only -- exactly on any input."""
import functools

import numpy as np

import geometry_ref as R

B = 2
LATTICE_CASES = ((257, 33), (300, 1023), (257, 1025), (513, 2500))     # (N, M): a partly dead last wave, one tile - 1, + 1, three tiles
KS = (1, 3, 4, 5, 16, 17, 32)                                          # every capacity, each boundary between two, K = M - 1 at M = 33
VOTE_CASE = (513, 2500)
VOTE_KS = (1, 5, 16, 32)
VOTE_CUTS = (np.inf, 3 / 64, 0.0)
N_LABELS = 32                                                          # labels 0 .. 31; the test lut holds 31 entries


@functools.lru_cache(maxsize=None)
def lattice_case(N, M):
    """(q [B,N,3], c [B,M,3], labels int64 [B,M]) of one lattice case; computed once, never modified."""
    rng = np.random.default_rng(1000 * N + M)
    q, c = R.lattice(rng, B, N), R.lattice(rng, B, M)
    labels = np.random.default_rng(7).integers(0, N_LABELS, (B, M)).astype(np.int64)
    for a in (q, c, labels):
        a.setflags(write=False)
    return q, c, labels


@functools.lru_cache(maxsize=None)
def lattice_sorted(N, M):
    """(stable argsort [B,N,M], sorted fp64 distances [B,N,M]) of a lattice case: every K's answer is a prefix of it."""
    q, c, _ = lattice_case(N, M)
    d = R.square_distance64(q, c)
    order = np.argsort(d, axis=-1, kind="stable")
    ds = np.take_along_axis(d, order, -1)
    order.setflags(write=False)
    ds.setflags(write=False)
    return order, ds


def knn64(q, c, K):
    """q [B,N,3] queries, c [B,M,3] candidates, K <= M -> (idx int64 [B,N,K], dist fp64 [B,N,K]): the first K of a STABLE
    argsort of the fp64 distances (equal distances in ascending candidate index) and the distances themselves."""
    d = R.square_distance64(q, c)
    idx = np.argsort(d, axis=-1, kind="stable")[..., :K]
    return idx.astype(np.int64), np.take_along_axis(d, idx, -1)


def vote_row(idx, dist, labels, M, max_d2):
    """One row: (winner, number of voters).  Slot k votes iff 0 <= idx[k] < M and not (dist[k] > max_d2); the winner is the
    label with the most voting slots, among labels with equally many the one whose first voting slot comes first."""
    count, first = {}, {}
    for k in range(len(idx)):
        i = int(idx[k])
        if 0 <= i < M and not (dist[k] > max_d2):
            lab = int(labels[i])
            count[lab] = count.get(lab, 0) + 1
            first.setdefault(lab, k)
    if not count:
        return None, 0
    return min(count, key=lambda lab: (-count[lab], first[lab])), sum(count.values())


def vote_ref(idx, dist, labels, M, max_d2, fill, lut=None, dst=None, out=None, out_stride=None, n_query=None):
    """idx / dist [B,N,K], labels int64 [B,M] -> (out int32 [B, out_stride], err): the rule of pn2_knn_vote.  ``out``: the
    buffer as it was before the call (rows that are not written keep their content); default: [B, N] of ``fill``."""
    B, N, _ = idx.shape
    out_stride = (N if out is None else out.shape[1]) if out_stride is None else out_stride
    out = np.full((B, out_stride), fill, np.int32) if out is None else np.array(out, np.int32).reshape(B, out_stride)
    err = 0
    for b in range(B):
        nq = N if n_query is None else min(max(int(n_query[b]), 0), N)
        for n in range(nq):
            win, voters = vote_row(idx[b, n], dist[b, n], labels[b], M, max_d2)
            res = fill
            if voters:
                if lut is None:
                    res = win
                elif 0 <= win < len(lut):
                    res = int(lut[win])
                else:
                    err |= 1
            pos = n
            if dst is not None:
                pos = int(dst[b, n])
                if not 0 <= pos < out_stride:
                    err |= 2
                    continue
            out[b, pos] = res
    return out, err


def has_tied_vote(idx, dist, labels, M, max_d2):
    """One row: do two different labels share the largest number of voting slots?"""
    count = {}
    for k in range(len(idx)):
        i = int(idx[k])
        if 0 <= i < M and not (dist[k] > max_d2):
            count[int(labels[i])] = count.get(int(labels[i]), 0) + 1
    top = sorted(count.values(), reverse=True)
    return len(top) > 1 and top[0] == top[1]
