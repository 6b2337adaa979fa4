"""GPU, end to end: registration.register_global on two overlapping, differently posed parts of one surface, then icp(init=...).

THE SCENE (corr_ransac_ref.bump_scene, shared and read-only): 3072 points on the height field of 12 Gaussian bumps over [-2,2]^2 with
analytic normals; target = the rows with x > -0.8 (M = 2127), source = the rows with x < 0.8 (N = 2199), permuted, rotated 140
degrees about (1,2,3) and translated.  k = 32, radius = 0.35, threshold = 0.05, search = "brute", the normals passed in.

THE CRITERION: every source row, moved by register_global's transform, lies within ``threshold`` of its true position -- the inlier
radius itself, the level at which RANSAC's answer counts as right, not a tuned constant.

THE REFERENCE'S OWN FIGURES on this scene, measured on the CPU with the committed numpy references (fpfh_ref with a fp64 self-search,
a fp64 nearest-feature matcher, corr_ransac_ref with the sampler above):
    nearest-feature matches within threshold of the truth        30.7 %
    rows kept by the mutual test                                  39.9 % (878 pairs); with the ratio test at 0.9 as well: 830
    of the mutual pairs, within threshold of the truth            74.5 % (78.1 % of the 830)
    valid hypotheses of 256 at edge_ratio 0.9                     113 (mutual pairs), 119 (mutual + ratio)
    count of the best hypothesis                                  657 of 878, 648 of 830
    largest source-row error of the best hypothesis itself        0.026 (H = 256, mutual), 1.8e-6 (mutual + ratio: an exact triple won)
    after one least-squares refit on its inliers (Horn; SVD-Kabsch gives the same three digits)     7.0e-4, 3.0e-4
    after two refits                                              5.7e-4, 5.3e-4;  the same with H = 1024: 5.7e-4, 5.3e-4
All of it sits two orders of magnitude below the criterion.  One run of this test on one MI355X (a record, not a bound): 830 pairs,
649 inliers, largest source-row error 5.27e-4 after register_global (the reference's figures for mutual + ratio, H = 1024) and
1.02e-5 after the 20 point-to-plane ICP steps that start from it."""
import numpy as np
import pytest
import torch

import corr_ransac_ref as C
from pointnet12_amd import _lib, registration

pytestmark = pytest.mark.gpu

K, RADIUS, THRESHOLD = 32, 0.35, 0.05


def cu(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def row_error(transform, scene, rows=None):
    """The largest distance of a source row, moved by ``transform`` ([4,4] float64), from its true position."""
    moved = C.apply(transform.cpu().numpy()[:3].reshape(12), scene["source"].astype(np.float64))
    e = np.linalg.norm(moved - scene["truth"], axis=1)
    return float(e.max() if rows is None else e[:rows].max())


def test_register_global_then_icp(dev):
    sc = C.bump_scene()
    src, tgt, ns, nt = (cu(sc[k], dev) for k in ("source", "target", "source_normals", "target_normals"))
    res = registration.register_global(src, tgt, RADIUS, threshold=THRESHOLD, k=K, normals=(ns, nt), search="brute")
    assert res.transform.shape == (4, 4) and int(res.status) == 0 and int(res.best_h) >= 0
    pairs, inliers = int(res.matches.count), int(res.count)
    err = row_error(res.transform, sc)
    print("register_global: %d pairs, %d inliers, rmse %.3g, largest source-row error %.3g" % (pairs, inliers, float(res.rmse), err))
    assert inliers >= 3 and inliers <= pairs <= len(sc["source"])
    assert err <= THRESHOLD
    again = registration.register_global(src, tgt, RADIUS, threshold=THRESHOLD, k=K, normals=(ns, nt), search="brute")
    assert torch.equal(again.transform.view(torch.int64), res.transform.view(torch.int64))          # two runs, the same bytes
    fine = registration.icp(src, tgt, THRESHOLD, metric="plane", init=res.transform, target_normals=nt, iterations=20)
    err_icp = row_error(fine.transform, sc)
    print("icp from it: fitness %.3f, rmse %.3g, largest source-row error %.3g" % (float(fine.fitness), float(fine.rmse), err_icp))
    assert err_icp <= THRESHOLD and float(fine.fitness) > 0.5
    lost = registration.icp(src, tgt, THRESHOLD, metric="plane", target_normals=nt, iterations=20)          # ICP alone, from the identity, is lost
    assert row_error(lost.transform, sc) > 10 * THRESHOLD


def _capture(step):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = step()
    return graph, res


def test_register_global_captures_and_follows_the_counts(dev):
    """register_global with buffers: captured once, replayed after the device-side counts changed, without an allocation; the
    replay's bytes are the eager call's at the same counts, and the changed count changes the pair list."""
    sc = C.bump_scene()
    N, M = len(sc["source"]), len(sc["target"])
    src, tgt, ns, nt = (cu(sc[k], dev)[None] for k in ("source", "target", "source_normals", "target_normals"))
    buf = registration.global_buffers(N, M, B=1, k=K, iterations=256, device=dev, search="brute")
    n_s, n_t = torch.tensor([N], device=dev), torch.tensor([M], device=dev)

    def step():
        return registration.register_global(src, tgt, RADIUS, threshold=THRESHOLD, k=K, normals=(ns, nt), search="brute", iterations=256,
                                            n_source=n_s, n_target=n_t, buffers=buf)

    graph, res = _capture(step)
    assert res.transform is buf.corr.transform and res.matches.count is buf.matches.count
    seen = []
    for rows_s, rows_t in ((N, M), (N - 400, M), (N, M - 300), (0, M)):
        n_s.fill_(rows_s)
        n_t.fill_(rows_t)
        buf.corr.transform[:, :3].zero_()                           # (the rows a call writes; the last row is the buffers' own 0 0 0 1)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
        replayed = (res.transform.clone(), res.count.clone(), res.matches.count.clone(), res.status.clone())
        eager = registration.register_global(src, tgt, RADIUS, threshold=THRESHOLD, k=K, normals=(ns, nt), search="brute", iterations=256,
                                             n_source=n_s, n_target=n_t)
        assert torch.equal(replayed[0].view(torch.int64), eager.transform.view(torch.int64))
        assert torch.equal(replayed[1], eager.count) and torch.equal(replayed[2], eager.matches.count) and torch.equal(replayed[3], eager.status)
        pairs = int(replayed[2])
        assert pairs <= rows_s and torch.equal(res.matches.pair_src[0, :pairs], eager.matches.pair_src[0, :pairs])
        seen.append(pairs)
        if rows_s == 0:
            assert pairs == 0 and int(replayed[3]) == _lib.CORR_NONE and torch.equal(replayed[0][0], torch.eye(4, device=dev, dtype=torch.float64))
            with pytest.raises(ValueError):
                buf.check(none_ok=False)
            buf.check()
        else:
            assert int(replayed[3]) == 0 and row_error(replayed[0][0], sc, rows_s) <= THRESHOLD
    assert len(set(seen)) == 4                                       # the replay followed the counts
