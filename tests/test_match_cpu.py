"""CPU: the tie and exclusion rules of tests/match_ref.py on integer-valued features, where equal distances are exact."""
import numpy as np

import match_ref as R


def test_ties_keep_index_order():
    f = np.float32([[1, 0], [0, 1], [1, 0], [3, 3], [0, 1]])[None]          # rows 0 and 2 equal, rows 1 and 4 equal
    q = np.float32([[1, 0], [0, 0.5], [3, 3]])[None]
    idx, dist = R.feature_nn2(q, f, 2)
    assert idx[0].tolist() == [[0, 2], [1, 4], [3, 0]]
    assert dist[0].tolist() == [[0, 0], [0.25, 0.25], [0, 13]]


def test_rows_that_take_no_part():
    f = np.float32([[0, 0, 9], [np.nan, 1, 9], [2, 2, 9], [np.inf, 0, 9], [2, 3, 9]])[None]          # D = 2: column 2 is not read
    q = np.float32([[2, 2, 0], [0, 0, 5], [np.nan, 0, 0], [1, 1, 0]])[None]
    idx, dist = R.feature_nn2(q, f, 2)
    assert idx[0].tolist() == [[2, 4], [5, 5], [5, 5], [2, 4]]
    assert dist[0, 0].tolist() == [0, 1] and np.isinf(dist[0, 1:3]).all() and dist[0, 3].tolist() == [2, 5]
    assert R.takes_part(f[0], 2).tolist() == [False, False, True, False, True]


def test_single_candidate_and_counts():
    f = np.float32([[1], [2], [3]])[None]
    q = np.float32([[1.25], [9]])[None]
    idx, dist = R.feature_nn2(q, f, 1, n_cand=[1])
    assert idx[0].tolist() == [[0, 3], [0, 3]] and dist[0, :, 0].tolist() == [0.0625, 64] and np.isinf(dist[0, :, 1]).all()
    idx, dist = R.feature_nn2(q, f, 1, n_query=[1], n_cand=[0], idx_before=np.full((1, 2, 2), -7), dist_before=np.full((1, 2, 2), -1.0))
    assert idx[0].tolist() == [[3, 3], [-7, -7]] and dist[0, 1].tolist() == [-1, -1]


def test_overflowing_distance_is_never_kept():
    f = np.float32([[3e38], [-3e38]])[None]
    q = np.float32([[-3e38]])[None]
    idx, dist = R.feature_nn2(q, f, 1)
    assert idx[0].tolist() == [[1, 2]] and np.isinf(dist[0, 0, 1])


def test_pairs_mutual_and_ratio():
    idx = np.int64([[[1, 0], [1, 2], [3, 3], [0, 1]]])                      # row 2 has no neighbour (M = 3)
    dist = np.float32([[[1, 2], [0, 0], [np.inf, np.inf], [4, np.inf]]])
    back = np.int64([[[3, 0], [1, 0], [9, 9]]])
    s, t, c = R.match_pairs(idx, dist, None, 3, np.inf)
    assert c.tolist() == [3] and s[0].tolist() == [0, 1, 3, -1] and t[0].tolist() == [1, 1, 0, -1]
    s, t, c = R.match_pairs(idx, dist, back, 3, np.inf)
    assert c.tolist() == [2] and s[0, :2].tolist() == [1, 3] and t[0, :2].tolist() == [1, 0]
    s, t, c = R.match_pairs(idx, dist, None, 3, 0.5)                         # 1 <= 0.5 * 2 passes, 0 <= 0 passes, a missing second passes
    assert c.tolist() == [3]
    s, t, c = R.match_pairs(idx, dist, None, 3, 0.25)
    assert c.tolist() == [2] and s[0, :2].tolist() == [1, 3]
    s, t, c = R.match_pairs(idx, dist, None, 3, 0.0)                         # only an exact match, or a row without a second neighbour
    assert s[0, :2].tolist() == [1, 3]
    s, t, c = R.match_pairs(idx, dist, None, 3, np.inf, n_query=[1])
    assert c.tolist() == [1] and s[0].tolist() == [0, -1, -1, -1]


def test_whole_matcher_on_a_permutation():
    rng = np.random.default_rng(1)
    ft = rng.integers(0, 50, (1, 40, 5)).astype(np.float32)
    perm = rng.permutation(40)
    fs = ft[:, perm] + np.float32(0.125)
    s, t, c, idx, dist = R.match_features(fs, ft, 5, mutual=True, ratio=0.9)
    assert c[0] > 30 and (t[0, :c[0]] == perm[s[0, :c[0]]]).all()
