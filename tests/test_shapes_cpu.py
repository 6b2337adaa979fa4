"""CPU: the host side of pointnet12_amd/shapes.py (readers, augmentation functions, caches, argument checks) and the numpy
restatement tests/shapes_ref.py, against what the REFERENCE produced (tests/golden/g17_shapes.npz, tools/make_golden_shapes.py)."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

import shapes_ref as SR
from conftest import GOLDEN, ROOT, golden
from pointnet12_amd import _lib, s3dis, shapes

TREE = os.path.join(GOLDEN, "g17_shapenet")
MNET = os.path.join(GOLDEN, "g17_modelnet")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return bool((bits(a) == bits(b)).all()) if a.dtype == np.float32 else bool(np.array_equal(a, b))


def rows7(name):
    return np.loadtxt(os.path.join(TREE, name)).astype(np.float32)


def test_restatement_reproduces_the_reference_shapenet_items():
    g = golden("g17_shapes.npz")
    seen_m, seen_n, seen_flags = set(), set(), set()
    for tag in g["shapenet/cases"]:
        np.random.seed(int(g[tag + "/seed"]))
        pc, cls, seg, normal = SR.shapenet_item(rows7(str(g[tag + "/file"])), int(g[tag + "/cls"][0]), int(g[tag + "/npoints"]),
                                                bool(g[tag + "/normalize"]), bool(g[tag + "/augment"]))
        assert same(pc, g[tag + "/points"]) and same(cls, g[tag + "/cls"]), tag
        assert same(seg, g[tag + "/seg"]) and same(normal, g[tag + "/normals"]), tag
        seen_m.add(int(g[tag + "/M"])); seen_n.add(int(g[tag + "/npoints"]))
        seen_flags.add((bool(g[tag + "/augment"]), bool(g[tag + "/normalize"])))
    assert seen_m >= {2, 63, 64, 65, 300} and seen_n >= {1, 64, 255, 257, 2048} and len(seen_flags) == 4


def test_restatement_reproduces_the_reference_modelnet_and_s3dis_items():
    g = golden("g17_shapes.npz")
    data, label = shapes.load_modelnet(MNET, train=False)
    for i in (0, 4):
        np.random.seed(int(g["modelnet/item%d/seed" % i]))
        assert same(SR.modelnet_item(data[i], label[i], True)[0], g["modelnet/item%d/augmented" % i]), i
        assert same(SR.modelnet_item(data[i], label[i], False)[0], data[i])
    d0, l0 = s3dis.load_h5(os.path.join(GOLDEN, "g11_s3dis", "ply_data_all_0.h5"))
    k = int(g["s3dis/block"])
    np.random.seed(int(g["s3dis/seed"]))
    assert same(SR.s3dis_item(d0[k], l0[k], True)[0], g["s3dis/jittered"])


def test_augmentation_functions_are_the_references_bit_for_bit():
    g = golden("g17_shapes.npz")
    for k in range(5):
        out = shapes.point_cloud_normalize(g["aug/normalize%d/in" % k])
        assert same(out, g["aug/normalize%d/out" % k]), k
    batch = g["aug/batch"]
    np.random.seed(41)
    assert same(shapes.rotate_point_cloud(batch), g["aug/rotate"])
    assert same(shapes.rotate_point_cloud_by_angle(batch, 1.25), g["aug/rotate_by_angle"])
    np.random.seed(42)
    jit = shapes.jitter_point_cloud(batch)
    assert jit.dtype == np.float64 and np.array_equal(jit.view(np.uint64), g["aug/jitter"].view(np.uint64))
    np.random.seed(43)
    d, l, idx = shapes.shuffle_data(batch, np.arange(3))
    assert same(d, g["aug/shuffle_data"]) and np.array_equal(l, g["aug/shuffle_labels"]) and np.array_equal(idx, g["aug/shuffle_idx"])


def test_shapenet_index_matches_the_reference():
    g = golden("g17_shapes.npz")
    for split in ("train", "val", "test", "trainval"):
        ds = shapes.ShapeNetPart(TREE, split, device=None)
        assert ["/".join(p.split(os.sep)[-2:]) for p in ds.datapath] == list(g["shapenet/%s/datapath" % split]), split
        assert len(ds) == int(g["shapenet/%s/len" % split])
        assert list(ds.classes.keys()) == list(g["shapenet/classes"]) and list(ds.classes.values()) == list(g["shapenet/class_ids"])
    with pytest.raises(ValueError) as e:
        shapes.ShapeNetPart(TREE, "bogus", device=None)
    assert str(e.value) == str(g["shapenet/unknown_split_message"])
    assert shapes.label_id_to_name[36] == "Mug" and shapes.seg_classes["Airplane"] == [0, 1, 2, 3]
    assert sorted(l for v in shapes.seg_classes.values() for l in v) == list(range(50))


def test_shapenet_rows_and_class_ids_match_the_recorded_items():
    """The rows the store would hold: normalised xyz (exact by construction: the numpy function itself) + normals."""
    g = golden("g17_shapes.npz")
    sets = {s: shapes.ShapeNetPart(TREE, s, device=None) for s in ("trainval", "test")}
    raw = {s: shapes.ShapeNetPart(TREE, s, normalize=False, device=None) for s in ("trainval", "test")}
    for tag in g["shapenet/cases"]:
        ds = (sets if bool(g[tag + "/normalize"]) else raw)[str(g[tag + "/split"])]
        i = int(g[tag + "/index"])
        assert "/".join(ds.datapath[i].split(os.sep)[-2:]) == str(g[tag + "/file"])
        assert ds.cls_ids[i] == g[tag + "/cls"][0]
        rows = ds.host_rows(i)
        assert rows.dtype == np.float32 and rows.shape == (int(g[tag + "/M"]), 6)
        if not bool(g[tag + "/augment"]):                       # every recorded row is one of the stored rows, bit for bit
            have = set(map(bytes, rows))
            got = np.concatenate([g[tag + "/points"], g[tag + "/normals"]], 1)
            assert all(bytes(r) in have for r in got), tag


def test_shapenet_npz_cache_round_trip(tmp_path):
    cache = str(tmp_path / "train.npz")
    a = shapes.ShapeNetPart(TREE, "train", cache=cache, device=None)
    assert os.path.exists(cache)
    before = os.path.getmtime(cache), os.path.getsize(cache)
    b = shapes.ShapeNetPart(TREE, "train", cache=cache, device=None)
    assert (os.path.getmtime(cache), os.path.getsize(cache)) == before
    assert len(a.arrays) == len(b.arrays) == 4
    for x, y in zip(a.arrays, b.arrays):
        assert same(x, y)
    with pytest.raises(ValueError):
        shapes.ShapeNetPart(TREE, "test", cache=cache, device=None)      # another split's cache is refused, not reused


def test_modelnet_files_read_bit_for_bit():
    g = golden("g17_shapes.npz")
    data, label = shapes.load_modelnet(MNET, train=False)
    assert data.dtype == np.float32 and data.shape == (5, 2048, 3) and label.dtype == np.uint8 and label.shape == (5, 1)
    assert np.array_equal(np.frombuffer(hashlib.sha256(data.tobytes()).digest(), np.uint8), g["modelnet/data_sha"])
    assert np.array_equal(label, g["modelnet/label"])
    ds = shapes.ModelNet40(MNET, train=False, device=None)
    assert len(ds) == 5 and len(ds.class_names) == 40 and ds.class_names[0] == "airplane" and ds.class_names[-1] == "xbox"
    with pytest.raises(FileNotFoundError):
        shapes.load_modelnet(MNET, train=True)                            # the fixture holds the two test files only


def test_entry_point_is_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "pn2.h")).read()
    assert re.search(r"\bint\s+pn2_prepare_shapes\s*\(", text)
    res, args = _lib.SIGNATURES["pn2_prepare_shapes"]
    assert res is ctypes.c_int and len(args) == 16
    assert _lib.load().pn2_version() == _lib.ABI_VERSION


def test_prepare_shapes_argument_checks_need_no_gpu():
    """Bad arguments return -1 before anything touches the device (the pointers are never dereferenced on the host)."""
    lib = _lib.load()
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data

    def call(raw=p, C=6, begin=p, count=p, rot=None, noise=None, noise_cols=3, B=2, N=4, out=p):
        return lib.pn2_prepare_shapes(raw, C, begin, count, None, rot, noise, noise_cols, None, None, B, N, out, None, None, None)
    assert call(raw=None) == -1 and call(begin=None) == -1 and call(count=None) == -1 and call(out=None) == -1
    assert call(C=2) == -1 and call(C=17) == -1
    assert call(noise=p, noise_cols=0) == -1 and call(noise=p, noise_cols=7) == -1 and call(noise=p, C=3, noise_cols=4) == -1
    assert call(B=0) == -1 and call(B=-1) == -1 and call(N=0) == -1 and call(N=-5) == -1
    assert call(raw=p + 2) == -1 and call(out=p + 1) == -1 and call(rot=p + 4) == -1
