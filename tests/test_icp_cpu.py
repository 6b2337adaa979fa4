"""CPU: the numpy statement of the ICP rule (tests/icp_ref.py) checks itself -- it recovers a planted transform on a zero-noise pair,
calls degenerate systems singular exactly at the stated counts -- and kitti.read_poses round-trips a file written here."""
import numpy as np
import pytest

import grid_knn_ref as R
import icp_ref as I


@pytest.mark.parametrize("metric", [I.PLANE, I.POINT])
def test_reference_recovers_the_planted_transform(metric):
    o, e_ref, cond = I.sheets_reference(metric)
    print("\nmetric %d: %d iterations, e_ref = %.3g, cond(A) = %.3g" % (metric, o["iters"][0], e_ref, cond))
    assert o["status"][0] == I.CONVERGED and 1 <= o["iters"][0] <= 30 and o["count"][0] == 1024
    assert cond <= 1e6
    # the source is the target under the inverse transform rounded to float32 (2^-24 of coordinates up to 2.5): 1e-6 is a loose ceiling
    assert e_ref <= 1e-6
    Rm = o["T"][0].reshape(3, 4)[:, :3]
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() <= o["iters"][0] * 2.0 ** -50


def one_step(metric, normals=None, n_src=None, T=None):
    src, tgt, nrm = I.sheets_pair()
    m = np.float32(I.SHEETS_MAX_DIST ** 2)
    return I.icp_step(src, tgt, nrm if normals is None else normals, I.PLANTED[None] if T is None else T, np.zeros(1, np.int32), np.zeros(1, np.int32),
                      m, 0.0, R.default_cell(m), metric, n_src=n_src)


def test_equal_normals_are_singular_for_plane():
    _, tgt, _ = I.sheets_pair()
    flat = np.broadcast_to(np.float32([0.0, 0.6, 0.8]), tgt.shape)
    o = one_step(I.PLANE, normals=flat)
    assert o["status"][0] == I.SINGULAR and o["err"] == I.ERR_SINGULAR and (o["x"][0] == 0).all() and o["iters"][0] == 0
    assert np.array_equal(o["T"][0], I.PLANTED) and o["count"][0] == 1024
    assert one_step(I.POINT, normals=flat)["status"][0] == 0                       # (the point metric does not read them)


@pytest.mark.parametrize("metric,least", [(I.PLANE, 6), (I.POINT, 3)])
def test_singular_exactly_below_the_stated_count(metric, least):
    o = one_step(metric, n_src=np.int64([least - 1]))
    assert o["count"][0] == least - 1 and o["status"][0] == I.SINGULAR and o["err"] == I.ERR_SINGULAR
    o = one_step(metric, n_src=np.int64([least]))
    assert o["count"][0] == least and o["status"][0] == 0 and o["err"] == 0 and o["iters"][0] == 1 and np.isfinite(o["x"]).all()


def test_eval_only_and_frozen_clouds_in_the_reference():
    src, tgt, nrm = I.sheets_pair()
    m = np.float32(I.SHEETS_MAX_DIST ** 2)
    for st in (I.CONVERGED, I.SINGULAR):
        o = I.icp_step(src, tgt, nrm, I.PLANTED[None], np.int32([st]), np.int32([7]), m, 0.0, R.default_cell(m), I.PLANE)
        assert not o["touched"][0] and o["count"][0] == -1 and (o["corr"] == -1).all() and o["iters"][0] == 7
        e = I.icp_step(src, tgt, None, I.PLANTED[None], np.int32([st]), np.int32([7]), m, 0.0, R.default_cell(m), I.POINT, flags=I.EVAL_ONLY)
        assert e["touched"][0] and e["count"][0] == 1024 and e["status"][0] == st and np.array_equal(e["T"][0], I.PLANTED)
        assert np.sqrt(e["sums"][0, 27] / 1024) < 1e-6                          # the planted transform puts every row on its target point


def test_read_poses_round_trip(tmp_path):
    from pointnet12_amd import kitti
    rng = np.random.default_rng(3)
    poses = np.tile(np.eye(4), (5, 1, 1))
    for f in range(5):
        poses[f, :3, :3] = I.rotation(rng.standard_normal(3), rng.uniform(-1, 1))
        poses[f, :3, 3] = rng.uniform(-50, 50, 3)
    fn = tmp_path / "poses.txt"
    with open(fn, "w") as fh:
        for P in poses:
            fh.write(" ".join(repr(float(v)) for v in P[:3].reshape(-1)) + "\n")
    got = kitti.read_poses(str(fn))
    assert got.dtype == np.float64 and got.shape == (5, 4, 4) and np.array_equal(got, poses)
    Tr = np.concatenate([I.rotation((1, -1, 0.5), 1.5), [[0.1], [-0.3], [0.2]]], 1)
    Tr4 = np.concatenate([Tr, [[0, 0, 0, 1]]])
    want = np.linalg.inv(Tr4) @ poses @ Tr4
    for form in (Tr, Tr4, Tr.reshape(-1)):
        assert np.array_equal(kitti.read_poses(str(fn), Tr=form), want)
    assert np.abs(want[:, 3] - [0, 0, 0, 1]).max() == 0
    with open(fn, "a") as fh:
        fh.write("1 2 3\n")
    with pytest.raises(ValueError):
        kitti.read_poses(str(fn))
