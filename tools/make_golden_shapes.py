#!/usr/bin/env python3
"""tests/golden/g17_shapes.npz, g17_shapenet/, g17_modelnet/: the REFERENCE's ShapeNet-part / ModelNet / S3DIS items, recorded.

    python tools/make_golden_shapes.py     # development container only: reads the reference and /opt/conda/lib/libhdf5.so

* Imports the reference's ``data_utils/augmentation.py`` and ``PartNormalDataset`` unmodified (a stub ``h5py`` / ``tqdm`` in
  ``sys.modules`` is enough: the class only needs the imports to succeed).
* Builds a tiny synthetic ShapeNet-part tree (3 categories, 8 files of 2 .. 300 points, the three split lists) and two
  ModelNet-layout files (``ply_data_test0.h5`` / ``ply_data_test1.h5``: ``data`` float32 [n, 2048, 3], ``label`` uint8 [n, 1],
  gzip-chunked as the originals) written by libhdf5 itself through ctypes.  All contents are synthetic.
* Runs the reference with fixed numpy seeds: ``PartNormalDataset.__getitem__`` (its cache filled with
  ``np.loadtxt(fn).astype(float32)``, the branch the reference takes on a hit) over M x npoints x augment x normalize cases;
  for ModelNet and S3DIS the augmentation their ``__getitem__`` intends and cannot run (NameError on ``pcd``), i.e.
  ``rotate_point_cloud`` / ``jitter_point_cloud(...).astype(float32)`` of the item with the reference's own functions.
* Before writing, asserts that tests/shapes_ref.py reproduces every recorded element bit for bit: a later GPU mismatch is
  then the kernel's.
"""
import ctypes
import json
import os
import shutil
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("PN2_REFERENCE", "/root/reference")
GOLD = os.path.join(ROOT, "tests", "golden")
TREE = os.path.join(GOLD, "g17_shapenet")
MNET = os.path.join(GOLD, "g17_modelnet")

for name in ("h5py", "tqdm"):
    if name not in sys.modules:
        try:
            __import__(name)
        except ImportError:
            m = types.ModuleType(name)
            m.tqdm = lambda it, *a, **k: it
            sys.modules[name] = m
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from data_utils import augmentation as A                      # noqa: E402  (the reference)
from data_utils.ShapeNetDataLoader import PartNormalDataset   # noqa: E402  (the reference)
from data_utils.ModelNetDataLoader import ModelNetDataLoader  # noqa: E402  (the reference)
import shapes_ref as SR                                       # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool((bits(a) == bits(b)).all()) if a.dtype == np.float32 else bool(np.array_equal(a, b))


def write_h5(path, arrays, chunks):
    lib = ctypes.CDLL("/opt/conda/lib/libhdf5.so")
    hid = ctypes.c_int64
    lib.H5open()
    gid = lambda name: hid.in_dll(lib, name).value
    for fn, res, args in [("H5Fcreate", hid, [ctypes.c_char_p, ctypes.c_uint, hid, hid]),
                          ("H5Screate_simple", hid, [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
                          ("H5Pcreate", hid, [hid]), ("H5Pset_chunk", ctypes.c_int, [hid, ctypes.c_int, ctypes.c_void_p]),
                          ("H5Pset_deflate", ctypes.c_int, [hid, ctypes.c_uint]),
                          ("H5Dcreate2", hid, [hid, ctypes.c_char_p, hid, hid, hid, hid, hid]),
                          ("H5Dwrite", ctypes.c_int, [hid, hid, hid, hid, hid, ctypes.c_void_p]),
                          ("H5Dclose", ctypes.c_int, [hid]), ("H5Sclose", ctypes.c_int, [hid]), ("H5Pclose", ctypes.c_int, [hid]),
                          ("H5Fclose", ctypes.c_int, [hid])]:
        getattr(lib, fn).restype, getattr(lib, fn).argtypes = res, args
    DCPL = gid("H5P_CLS_DATASET_CREATE_ID_g")
    F32, U8 = gid("H5T_IEEE_F32LE_g"), gid("H5T_STD_U8LE_g")
    f = lib.H5Fcreate(path.encode(), 2, 0, 0)                      # H5F_ACC_TRUNC
    assert f >= 0
    for name, a in arrays.items():
        dims = (ctypes.c_uint64 * a.ndim)(*a.shape)
        sp = lib.H5Screate_simple(a.ndim, dims, None)
        pl = lib.H5Pcreate(DCPL)
        c = (ctypes.c_uint64 * a.ndim)(*chunks[name])
        assert lib.H5Pset_chunk(pl, a.ndim, c) >= 0
        assert lib.H5Pset_deflate(pl, 4 if a.dtype == np.float32 else 1) >= 0
        t = F32 if a.dtype == np.float32 else U8
        d = lib.H5Dcreate2(f, name.encode(), t, sp, 0, pl, 0)
        assert d >= 0
        a = np.ascontiguousarray(a)
        assert lib.H5Dwrite(d, t, 0, 0, 0, a.ctypes.data_as(ctypes.c_void_p)) >= 0
        lib.H5Dclose(d); lib.H5Pclose(pl); lib.H5Sclose(sp)
    lib.H5Fclose(f)


# (category, wordnet id, [(token, M, split)]) -- the order of synsetoffset2category.txt is NOT alphabetical, as in the original
TREE_SPEC = [("Mug", "03797390", [("b7e705de46ebdcc14af54ba5738cb1c5", 300, "train"), ("10c2b3eac377b9084b3c42e318f3affc", 2, "train"),
                                  ("c0c130c04edabc657c2b66248f91b3d8", 17, "test")]),
             ("Airplane", "02691156", [("1a04e3eab45ca15dd86060f189eb133", 63, "train"), ("2c1fff0653854166e7a636089598229", 64, "val"),
                                       ("3db61220251b3c9de719b5362fe06bbb", 65, "train")]),
             ("Cap", "02954340", [("90c6bffdc81cedbeb80102c6e0a7618a", 128, "test"), ("5eb9ab53213f5fff4e09ebaf49b0cb2f", 5, "val")])]
SEG_OF = {"Mug": [36, 37], "Airplane": [0, 1, 2, 3], "Cap": [6, 7]}

# (M, npoints, augment, normalize): every M and every npoints of the issue twice, the four augment x normalize settings spread
CASES = [(2, 1, True, True), (2, 257, False, True), (63, 64, True, False), (63, 2048, False, False), (64, 255, True, True),
         (64, 1, False, False), (65, 257, True, True), (65, 64, False, True), (300, 2048, True, True), (300, 255, False, False),
         (17, 64, True, True), (128, 255, True, False)]


def build_tree(rng):
    if os.path.isdir(TREE):
        shutil.rmtree(TREE)
    os.makedirs(os.path.join(TREE, "train_test_split"))
    lists = {"train": [], "val": [], "test": []}
    with open(os.path.join(TREE, "synsetoffset2category.txt"), "w") as f:
        for cat, wid, _ in TREE_SPEC:
            f.write("%s\t%s\n" % (cat, wid))
    for cat, wid, files in TREE_SPEC:
        os.makedirs(os.path.join(TREE, wid))
        for token, M, split in files:
            xyz = rng.uniform(-0.4, 0.4, (M, 3)) * np.array([1.0, 0.5, 0.25]) + np.array([0.05, -0.02, 0.1])
            nrm = rng.normal(size=(M, 3))
            nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
            seg = rng.choice(SEG_OF[cat], M).astype(np.float64)
            np.savetxt(os.path.join(TREE, wid, token + ".txt"), np.concatenate([xyz, nrm, seg[:, None]], 1), fmt="%.6f")
            lists[split].append("shape_data/%s/%s" % (wid, token))
    for split, names in lists.items():
        with open(os.path.join(TREE, "train_test_split", "shuffled_%s_file_list.json" % split), "w") as f:
            json.dump(names[::-1], f)


def main():
    rng = np.random.default_rng(17)
    out = {}
    build_tree(rng)

    # ---- ShapeNet-part: the reference's dataset object per split
    cache = {}
    m_of = {}
    for split in ("train", "val", "test", "trainval"):
        ds = PartNormalDataset(TREE, cache=cache, npoints=7, split=split)
        out["shapenet/%s/datapath" % split] = np.array(["/".join(p.split("/")[-2:]) for p in ds.datapath])
        out["shapenet/%s/len" % split] = np.int64(len(ds))
        for fn in ds.datapath:
            parts = fn.split("/")
            cache["%s_%s" % (parts[-2], parts[-1].split(".")[0])] = np.loadtxt(fn).astype(np.float32)
    out["shapenet/classes"] = np.array(list(ds.classes.keys()))
    out["shapenet/class_ids"] = np.array(list(ds.classes.values()), np.int64)
    try:
        PartNormalDataset(TREE, cache=cache, split="bogus")
        raise AssertionError("the reference accepted an unknown split")
    except ValueError as e:
        out["shapenet/unknown_split_message"] = np.array(str(e))
    full = PartNormalDataset(TREE, cache=cache, split="trainval")
    rel = ["/".join(p.split("/")[-2:]) for p in full.datapath]
    test = PartNormalDataset(TREE, cache=cache, split="test")
    tags = []
    for k, (M, npoints, augment, normalize) in enumerate(CASES):
        ds = None
        for cand in (full, test):
            for i, fn in enumerate(cand.datapath):
                parts = fn.split("/")
                if len(cache["%s_%s" % (parts[-2], parts[-1].split(".")[0])]) == M:
                    ds, index = cand, i
        assert ds is not None, M
        ds.npoints, ds.normalize, ds.data_augmentation = npoints, normalize, augment
        seed = 1700 + k
        np.random.seed(seed)
        pc, cls, seg, normal = ds[index]
        assert pc.dtype == np.float32 and normal.dtype == np.float32 and seg.dtype == np.int32 and cls.dtype == np.int32
        fn = ds.datapath[index]
        parts = fn.split("/")
        rows7 = cache["%s_%s" % (parts[-2], parts[-1].split(".")[0])]
        np.random.seed(seed)
        r = SR.shapenet_item(rows7, int(cls[0]), npoints, normalize, augment)
        assert same(r[0], pc) and same(r[1], cls) and same(r[2], seg) and same(r[3], normal), \
            "tests/shapes_ref.py differs from the reference on case %s" % (CASES[k],)
        tag = "shapenet/case%02d" % k
        tags.append(tag)
        out[tag + "/split"] = np.array("trainval" if ds is full else "test")
        out[tag + "/index"] = np.int64(index)
        out[tag + "/file"] = np.array("/".join(parts[-2:]))
        out[tag + "/M"], out[tag + "/npoints"], out[tag + "/seed"] = np.int64(M), np.int64(npoints), np.int64(seed)
        out[tag + "/augment"], out[tag + "/normalize"] = np.bool_(augment), np.bool_(normalize)
        out[tag + "/points"], out[tag + "/cls"], out[tag + "/seg"], out[tag + "/normals"] = pc, cls, seg, normal
    out["shapenet/cases"] = np.array(tags)

    # ---- the augmentation functions by themselves
    for k, M in enumerate((1, 2, 3, 64, 300)):
        pc = (rng.uniform(-1, 1, (M, 3)) * np.array([2.0, 1.0, 0.5]) + 0.3).astype(np.float32)
        out["aug/normalize%d/in" % k] = pc
        out["aug/normalize%d/out" % k] = A.point_cloud_normalize(pc)
        assert same(SR.normalize(pc), out["aug/normalize%d/out" % k]), M
    batch = rng.uniform(-1, 1, (3, 65, 3)).astype(np.float32)
    out["aug/batch"] = batch
    np.random.seed(41)
    out["aug/rotate"] = A.rotate_point_cloud(batch)
    np.random.seed(41)
    for b in range(3):
        assert same(SR.rotate(batch[b], np.random.uniform() * 2 * np.pi), out["aug/rotate"][b])
    out["aug/rotate_by_angle"] = A.rotate_point_cloud_by_angle(batch, 1.25)
    np.random.seed(42)
    out["aug/jitter"] = A.jitter_point_cloud(batch)
    assert out["aug/jitter"].dtype == np.float64
    np.random.seed(43)
    d, l, idx = A.shuffle_data(batch, np.arange(3))
    out["aug/shuffle_data"], out["aug/shuffle_labels"], out["aug/shuffle_idx"] = d, l, idx

    # ---- ModelNet: two files in the original layout
    if os.path.isdir(MNET):
        shutil.rmtree(MNET)
    os.makedirs(MNET)
    datas, labels = [], []
    for i, n in enumerate((3, 2)):
        d = rng.uniform(-1, 1, (n, 2048, 3)).astype(np.float32)
        d[0, :4] = np.array([[0, 0, 0], [0, 0.5, 0], [0.25, 0, 0], [0, 0, -0.75]], np.float32)     # exact zeros meet the rotation
        l = rng.integers(0, 40, (n, 1)).astype(np.uint8)
        write_h5(os.path.join(MNET, "ply_data_test%d.h5" % i), {"data": d, "label": l}, {"data": (1, 2048, 3), "label": (n, 1)})
        datas.append(d); labels.append(l)
    data, label = np.concatenate(datas), np.concatenate(labels)
    from pointnet12_amd import s3dis
    for i in range(2):
        rd, rl = s3dis.read_datasets(os.path.join(MNET, "ply_data_test%d.h5" % i), ("data", "label"))
        assert same(rd, datas[i]) and same(rl, labels[i])
    out["modelnet/data_sha"] = np.frombuffer(__import__("hashlib").sha256(data.tobytes()).digest(), np.uint8)
    out["modelnet/label"] = label
    plain = ModelNetDataLoader(data, label)
    for i in (0, 4):
        pc, lab = plain[i]
        assert same(pc, data[i]) and same(SR.modelnet_item(data[i], label[i])[0], pc)
        seed = 1800 + i
        np.random.seed(seed)
        pcd = np.expand_dims(data[i], axis=0)                      # ModelNetDataLoader.py:65-68 with the name it means
        pcd = A.rotate_point_cloud(pcd)
        pcd = A.jitter_point_cloud(pcd).astype(np.float32)
        pcd = np.squeeze(pcd, axis=0)
        np.random.seed(seed)
        assert same(SR.modelnet_item(data[i], label[i], True)[0], pcd), "tests/shapes_ref.py differs on ModelNet item %d" % i
        out["modelnet/item%d/seed" % i] = np.int64(seed)
        out["modelnet/item%d/augmented" % i] = pcd

    # ---- S3DIS: block 0 of the g11 fixture, jittered by the reference's function
    d0, l0 = s3dis.load_h5(os.path.join(GOLD, "g11_s3dis", "ply_data_all_0.h5"))
    np.random.seed(1900)
    jit = A.jitter_point_cloud(d0[1][None]).astype(np.float32)[0]
    np.random.seed(1900)
    assert same(SR.s3dis_item(d0[1], l0[1], True)[0], jit)
    np.random.seed(1900)
    from pointnet12_amd.s3dis import S3DISDataLoader
    assert same(S3DISDataLoader(d0, l0, True)[1][0], jit)
    out["s3dis/block"], out["s3dis/seed"], out["s3dis/jittered"] = np.int64(1), np.int64(1900), jit

    path = os.path.join(GOLD, "g17_shapes.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(tags), "ShapeNet cases, every element reproduced by tests/shapes_ref.py")
    for d in (TREE, MNET):
        for r, _, fs in os.walk(d):
            for f in fs:
                print("  %7d  %s" % (os.path.getsize(os.path.join(r, f)), os.path.relpath(os.path.join(r, f), GOLD)))


if __name__ == "__main__":
    main()
