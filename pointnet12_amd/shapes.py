"""Per-batch preparation of ShapeNet-part, ModelNet40 and S3DIS items on the HIP library.

The reference prepares every item of these three datasets on the host:

* ``PartNormalDataset.__getitem__`` (data_utils/ShapeNetDataLoader.py:95-127) on a cached ``[M, 7]`` float32 array
  (x y z nx ny nz seg): ``point_cloud_normalize`` (:113-114), with augmentation ``rotate_point_cloud`` then
  ``jitter_point_cloud(...).astype(float32)`` (:116-120), then ``np.random.choice(M, npoints, replace=True)`` and three
  fancy-index gathers (:123-126).  The normals are not rotated; duplicates of a raw point share their jitter.
* ``ModelNetDataLoader.__getitem__`` (data_utils/ModelNetDataLoader.py:60-70): ``data[i], label[i]``.  Its augmentation
  branch names a variable that does not exist (``pcd``, :65) and never stores its result: as shipped, augmentation raises
  ``NameError``.  Here it does what the branch plainly intends -- rotate then jitter of the item, the draws in the order
  ``uniform()``, ``randn(1, 2048, 3)`` -- and that is this project's reading, not the reference's behaviour.
* ``S3DISDataLoader.__getitem__``: the item ``s3dis.S3DISDataLoader`` states, ``(block + clip(0.01 * randn(4096, 9),
  +-0.05)).astype(float32)``.

Here the clouds stay resident in HBM (``ShapeStore``: all of ShapeNet-part is ~1.1 GB as [M, 6] rows) and one
``pn2_prepare_shapes`` launch writes the ``[B, N, C]`` batch and its ``[B, N]`` labels.  The normalisation is
deterministic and runs once, at fill time, with the numpy function itself.

Sources of the draws (``rng``):
  * ``"numpy"`` (default): numpy's global generator, cloud by cloud in the reference's order -- angle, noise, choice (the
    choice only when ``npoints`` is given) -- so ``np.random.seed(s)`` reproduces a ``num_workers=0`` loader bit for bit
    (worker processes reseed numpy in the reference as well).
  * a device ``torch.Generator``: the draws are made on the device (same distributions, another stream); only the ids
    cross PCIe.
  * a ``Draws`` tuple (``draw(...)`` makes one): device tensors that are used as they are, nothing crosses PCIe and
    nothing but the kernel is enqueued -- the form a captured step replays.
"""
import collections
import json
import os

import numpy as np
import torch

from . import _lib
from . import s3dis as _s3dis

_p = _lib.ptr


# ---- data_utils/augmentation.py, name for name (host, numpy) ------------------------------------------------------------
def point_cloud_normalize(pc):
    """augmentation.py:4-9."""
    centroid = np.mean(pc, axis=0)
    pc = pc - centroid
    m = np.max(np.sqrt(np.sum(pc ** 2, axis=1)))
    pc = pc / m
    return pc


def shuffle_data(data, labels):
    """augmentation.py:12-22: ``(data[idx], labels[idx], idx)`` for one ``np.random.shuffle`` of the indices."""
    idx = np.arange(len(labels))
    np.random.shuffle(idx)
    return data[idx, ...], labels[idx], idx


def rotate_point_cloud_by_angle(batch_data, rotation_angle):
    """augmentation.py:48-67: every cloud of ``[B, N, 3]`` about the up axis by one angle; float32 out."""
    assert len(batch_data.shape) == 3, batch_data.shape
    rotated_data = np.zeros(batch_data.shape, dtype=np.float32)
    for k in range(batch_data.shape[0]):
        cosval = np.cos(rotation_angle)
        sinval = np.sin(rotation_angle)
        rotation_matrix = np.array([[cosval, 0, sinval], [0, 1, 0], [-sinval, 0, cosval]])
        rotated_data[k, ...] = np.dot(batch_data[k, ...].reshape((-1, 3)), rotation_matrix)
    return rotated_data


def rotate_point_cloud(batch_data):
    """augmentation.py:25-45: one ``np.random.uniform()`` angle per cloud of ``[B, N, 3]``; float32 out."""
    assert len(batch_data.shape) == 3, batch_data.shape
    rotated_data = np.zeros(batch_data.shape, dtype=np.float32)
    for k in range(batch_data.shape[0]):
        rotation_angle = np.random.uniform() * 2 * np.pi
        rotated_data[k:k + 1] = rotate_point_cloud_by_angle(batch_data[k:k + 1], rotation_angle)
    return rotated_data


def jitter_point_cloud(batch_data, sigma=0.01, clip=0.05):
    """augmentation.py:70-82: float64 out (the callers cast)."""
    assert len(batch_data.shape) == 3, batch_data.shape
    B, N, C = batch_data.shape
    assert (clip > 0)
    jittered_data = np.clip(sigma * np.random.randn(B, N, C), -1 * clip, clip)
    jittered_data += batch_data
    return jittered_data


# ---- resident store -----------------------------------------------------------------------------------------------------
class ShapeStore:
    """Clouds ``[M_i, C]`` fp32 (a list, or one ``[n, P, C]`` array), 3 <= C <= 16, uploaded once and kept back to back in
    HBM; ``point_labels`` (one int array per cloud, or ``[n, P]``) and ``cloud_labels`` (``[n]``) ride along."""

    def __init__(self, clouds, point_labels=None, cloud_labels=None, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.Pn2Error("ShapeStore: the HIP device is the only implementation")
        if isinstance(clouds, np.ndarray) and clouds.ndim == 3:
            counts = [int(clouds.shape[1])] * int(clouds.shape[0])
            flat = clouds.reshape(-1, clouds.shape[2])
            if point_labels is not None:
                point_labels = np.asarray(point_labels).reshape(len(counts), -1)
        else:
            clouds = list(clouds)
            for c in clouds:
                if c.ndim != 2 or c.shape[1] != clouds[0].shape[1]:
                    raise ValueError("ShapeStore: clouds must be [M, C] arrays of one width")
            counts = [int(c.shape[0]) for c in clouds]
            flat = np.concatenate(clouds, 0) if clouds else None
        if not counts:
            raise ValueError("ShapeStore: no clouds")
        self.C = int(flat.shape[1])
        if not 3 <= self.C <= 16:
            raise ValueError("ShapeStore: rows of 3 .. 16 columns, got %d" % self.C)
        self.row_count = torch.tensor(counts, dtype=torch.int64)
        self.row_begin = torch.cumsum(self.row_count, 0) - self.row_count
        self.raw = torch.from_numpy(np.ascontiguousarray(flat, np.float32)).to(self.device)
        self.label = None
        if point_labels is not None:
            if [int(np.asarray(l).shape[0]) for l in point_labels] != counts:
                raise ValueError("ShapeStore: point_labels do not match the clouds row for row")
            lab = np.concatenate([np.asarray(l).reshape(-1) for l in point_labels], 0)
            self.label = torch.from_numpy(np.ascontiguousarray(lab, np.int32)).to(self.device)
        self.cloud_label = None
        if cloud_labels is not None:
            cl = np.asarray(cloud_labels).reshape(-1)
            if len(cl) != len(counts):
                raise ValueError("ShapeStore: one cloud label per cloud")
            self.cloud_label = torch.from_numpy(cl.astype(np.int64)).to(self.device)
        self._begin_dev = self.row_begin.to(self.device)
        self._count_dev = self.row_count.to(self.device)

    def __len__(self):
        return self.row_count.numel()


Draws = collections.namedtuple("Draws", "ids begin count rot noise noise_begin choice noise_cols")
Draws.__doc__ = """The device-resident arguments of one ``pn2_prepare_shapes`` launch: ``ids`` int64[B], ``begin`` / ``count``
int64[B] (the clouds' rows in the store), ``rot`` fp64[B, 2] (cos, sin) | None, ``noise`` fp64[*, noise_cols] | None with
``noise_begin`` int64[B], ``choice`` int64[B, N] | None."""


def draw(store, ids, npoints=None, rotate=False, jitter=False, noise_cols=3, rng="numpy", sigma=0.01, clip=0.05):
    """The random draws of a batch as a ``Draws`` of device tensors (see the module docstring for ``rng``)."""
    ids = torch.as_tensor(ids, dtype=torch.int64).reshape(-1).cpu()
    B = ids.numel()
    if B == 0:
        raise ValueError("prepare_shapes: empty batch")
    if jitter and not 1 <= noise_cols <= store.C:
        raise ValueError("prepare_shapes: noise_cols must be in 1 .. %d" % store.C)
    counts = store.row_count[ids]
    dev = store.device
    rot = noise = noise_begin = choice = None
    if isinstance(rng, str) and rng == "numpy":
        angles, rows, picks = [], [], []
        for m in counts.tolist():
            if rotate:
                angles.append(np.random.uniform() * 2 * np.pi)                    # augmentation.py:36
            if jitter:
                rows.append(np.clip(sigma * np.random.randn(1, m, noise_cols), -1 * clip, clip)[0])    # :80
            if npoints is not None:
                picks.append(np.random.choice(m, npoints, replace=True))          # ShapeNetDataLoader.py:123
        if rotate:
            a = np.asarray(angles, np.float64)
            rot = torch.from_numpy(np.stack([np.cos(a), np.sin(a)], 1)).to(dev)
        if jitter:
            noise = torch.from_numpy(np.concatenate(rows, 0)).to(dev)
        if npoints is not None:
            choice = torch.from_numpy(np.stack(picks).astype(np.int64)).to(dev)
    elif isinstance(rng, torch.Generator):
        cnt = counts.to(dev)
        if rotate:
            a = torch.rand(B, device=dev, dtype=torch.float64, generator=rng) * (2 * np.pi)
            rot = torch.stack([torch.cos(a), torch.sin(a)], 1).contiguous()
        if jitter:
            noise = torch.randn(int(counts.sum()), noise_cols, device=dev, dtype=torch.float64,
                                generator=rng).mul_(sigma).clamp_(-clip, clip)
        if npoints is not None:
            u = torch.rand(B, npoints, device=dev, dtype=torch.float64, generator=rng)
            choice = torch.minimum((u * cnt[:, None]).long(), cnt[:, None] - 1)
    else:
        raise ValueError('prepare_shapes: rng must be "numpy", a device torch.Generator or a Draws')
    if jitter:
        noise_begin = (torch.cumsum(counts, 0) - counts).to(dev)
    ids_dev = ids.to(dev)
    return Draws(ids_dev, store._begin_dev[ids_dev], store._count_dev[ids_dev], rot, noise, noise_begin, choice,
                 noise_cols if jitter else 0)


def prepare_shapes(store, ids, npoints=None, rotate=False, jitter=False, noise_cols=3, rng="numpy", out=None):
    """Batch of ``len(ids)`` clouds: ``(out [B, N, C] fp32, point_labels [B, N] int64 | None, cloud_labels [B] int64 |
    None)`` on the device.  ``npoints=None`` takes the first N = min(row_count) rows of every cloud as they are (ModelNet
    items, S3DIS blocks); otherwise N = npoints rows are drawn with replacement.  ``rotate`` turns columns 0..2 about the
    up axis, ``jitter`` adds clipped noise to columns < ``noise_cols``; every other column is copied.  ``rng`` is a
    ``Draws``: ``ids``, ``npoints``, ``rotate``, ``jitter`` and ``noise_cols`` are taken from it (pass ``ids=None``).
    ``out``: a ``(out, point_labels, cloud_labels)`` triple of contiguous tensors to write into (the static inputs of a
    captured step; labels may be None)."""
    lib, st = _lib.load(), _lib.stream()
    if isinstance(rng, Draws):
        d = rng
        if d.choice is None and npoints is None:
            raise ValueError("prepare_shapes: Draws without a choice need npoints (the rows taken from every cloud)")
        N = int(d.choice.shape[1]) if d.choice is not None else int(npoints)
    else:
        ids = torch.as_tensor(ids, dtype=torch.int64).reshape(-1).cpu()
        d = draw(store, ids, npoints, rotate, jitter, noise_cols, rng)
        N = int(npoints) if npoints is not None else int(store.row_count[ids].min())
    B, C, dev = d.ids.numel(), store.C, store.device
    if out is not None:
        points, labels, cls = out
        if points.shape != (B, N, C) or points.dtype != torch.float32 or not points.is_contiguous() or \
                (labels is not None and (labels.shape != (B, N) or labels.dtype != torch.int64 or not labels.is_contiguous())) or \
                (cls is not None and (cls.shape != (B,) or cls.dtype != torch.int64)):
            raise ValueError("prepare_shapes: out must be contiguous ([B, N, %d] float32, [B, N] int64, [B] int64)" % C)
        if (labels is not None and store.label is None) or (cls is not None and store.cloud_label is None):
            raise ValueError("prepare_shapes: the store holds no such labels")
        if cls is not None:
            torch.index_select(store.cloud_label, 0, d.ids, out=cls)
    else:
        points = torch.empty(B, N, C, device=dev, dtype=torch.float32)
        labels = torch.empty(B, N, device=dev, dtype=torch.int64) if store.label is not None else None
        cls = store.cloud_label[d.ids] if store.cloud_label is not None else None
    _lib.check(lib.pn2_prepare_shapes(_p(store.raw), C, _p(d.begin), _p(d.count), _p(store.label), _p(d.rot), _p(d.noise),
                                      d.noise_cols, _p(d.noise_begin), _p(d.choice), B, N, _p(points), _p(labels), None, st),
               "pn2_prepare_shapes")
    if out is not None:
        from . import pointnet_util as _U
        _U.bump_data_generation()             # a static buffer was refilled through a raw pointer: views of it are stale
    return points, labels, cls


# ---- ShapeNet-part ------------------------------------------------------------------------------------------------------
seg_classes = {'Earphone': [16, 17, 18], 'Motorbike': [30, 31, 32, 33, 34, 35], 'Rocket': [41, 42, 43], 'Car': [8, 9, 10, 11],
               'Laptop': [28, 29], 'Cap': [6, 7], 'Skateboard': [44, 45, 46], 'Mug': [36, 37], 'Guitar': [19, 20, 21],
               'Bag': [4, 5], 'Lamp': [24, 25, 26, 27], 'Table': [47, 48, 49], 'Airplane': [0, 1, 2, 3], 'Pistol': [38, 39, 40],
               'Chair': [12, 13, 14, 15], 'Knife': [22, 23]}                      # ShapeNetDataLoader.py:14-31
label_id_to_name = {label: cat for cat in seg_classes for label in seg_classes[cat]}


def shapenet_index(root, split):
    """``(datapath, classes, category)`` exactly as ``PartNormalDataset.__init__`` builds them (ShapeNetDataLoader.py:46-86):
    categories in the order of ``synsetoffset2category.txt``, each directory's files sorted and filtered by the split."""
    category = {}
    with open(os.path.join(root, 'synsetoffset2category.txt'), 'r') as f:
        for line in f:
            line = line.strip().split()
            category[line[0]] = line[1]
    fn_split = os.path.join(root, 'train_test_split')
    ids = {}
    for name in ("train", "val", "test"):
        with open(os.path.join(fn_split, 'shuffled_%s_file_list.json' % name), 'r') as f:
            ids[name] = set([str(d.split('/')[2]) for d in json.load(f)])
    if split == 'trainval':
        keep = ids["train"] | ids["val"]
    elif split in ids:
        keep = ids[split]
    else:
        raise ValueError('Unknown split: %s. Exiting..' % (split))
    datapath = []
    for item in category:
        dir_point = os.path.join(root, category[item])
        datapath += [os.path.join(dir_point, fn) for fn in sorted(os.listdir(dir_point)) if fn[0:-4] in keep]
    classes = dict(zip(category, range(len(category))))
    return datapath, classes, category


class ShapeNetPart:
    """``PartNormalDataset`` (ShapeNetDataLoader.py:37-130) with its items prepared on the device.  ``root`` is the
    ``shapenetcore_partanno_segmentation_benchmark_v0_normal`` directory; every file of the split is parsed with
    ``np.loadtxt(...).astype(float32)`` (x y z nx ny nz seg), xyz normalised once with ``point_cloud_normalize`` when
    ``normalize``, and the ``[M, 6]`` rows, the seg column and the class ids uploaded into a ``ShapeStore``.
    ``cache``: path of an ``.npz`` in this project's own format holding the parsed arrays of this root and split (written
    when missing, read when present -- parsing the 16 881 text files takes minutes)."""

    def __init__(self, root, split='train', npoints=2500, normalize=True, cache=None, device="cuda"):
        self.root, self.split, self.npoints, self.normalize = root, split, npoints, normalize
        self.datapath, self.classes, self.category = shapenet_index(root, split)
        self.wordnet_id_to_category = {v: k for k, v in self.category.items()}
        self.seg_classes = seg_classes
        names = ["/".join(fn.split(os.sep)[-2:]) for fn in self.datapath]
        arrays = self._read_cache(cache, names) if cache is not None and os.path.exists(cache) else None
        if arrays is None:
            arrays = [np.loadtxt(fn).astype(np.float32).reshape(-1, 7) for fn in self.datapath]
            if cache is not None:
                counts = np.array([len(a) for a in arrays], np.int64)
                np.savez(cache, format=np.array("pointnet12_amd.shapenet.v1"), names=np.array(names), counts=counts,
                         rows=np.concatenate(arrays, 0) if arrays else np.zeros((0, 7), np.float32))
        self.arrays = arrays
        self.cls_ids = np.array([self.classes[self.wordnet_id_to_category[n.split("/")[0]]] for n in names], np.int32)
        self.store = None
        if arrays and device is not None:
            self.store = ShapeStore([self.host_rows(i) for i in range(len(arrays))], [a[:, -1].astype(np.int32) for a in arrays],
                                    self.cls_ids, device)

    @staticmethod
    def _read_cache(path, names):
        with np.load(path) as z:
            if str(z["format"]) != "pointnet12_amd.shapenet.v1" or list(z["names"]) != names:
                raise ValueError("%s: not the cache of this root and split" % path)
            counts, rows = z["counts"], z["rows"]
        ends = np.cumsum(counts)
        return [rows[e - c:e] for c, e in zip(counts, ends)]

    def host_rows(self, index):
        """The ``[M, 6]`` rows of one shape as the store holds them: (normalised) xyz, then the normals."""
        a = self.arrays[index]
        xyz = point_cloud_normalize(a[:, 0:3]) if self.normalize else a[:, 0:3]
        return np.concatenate([xyz, a[:, 3:6]], 1).astype(np.float32)

    def __len__(self):
        return len(self.datapath)

    def batch(self, ids, augment=False, rng="numpy", out=None):
        """``(points [B, n, 3], cls [B], seg [B, n], normals [B, n, 3])`` on the device: views of one ``prepare_shapes``
        call (``points.transpose(2, 1)`` is what partseg.py feeds the network)."""
        o, seg, cls = prepare_shapes(self.store, ids, self.npoints, rotate=augment, jitter=augment, noise_cols=3, rng=rng, out=out)
        return o[..., 0:3], cls, seg, o[..., 3:6]


# ---- ModelNet40 ---------------------------------------------------------------------------------------------------------
class_names = ['airplane', 'bathtub', 'bed', 'bench', 'bookshelf', 'bottle', 'bowl', 'car', 'chair', 'cone', 'cup', 'curtain',
               'desk', 'door', 'dresser', 'flower_pot', 'glass_box', 'guitar', 'keyboard', 'lamp', 'laptop', 'mantel', 'monitor',
               'night_stand', 'person', 'piano', 'plant', 'radio', 'range_hood', 'sink', 'sofa', 'stairs', 'stool', 'table',
               'tent', 'toilet', 'tv_stand', 'vase', 'wardrobe', 'xbox']          # ModelNetDataLoader.py:8-13


def load_modelnet(path, train=True):
    """``(data [n, 2048, 3] float32, label [n, 1] uint8)`` of ``ply_data_train{0..4}.h5`` (train) or
    ``ply_data_test{0,1}.h5`` under the directory ``path``, concatenated in that order (ModelNetDataLoader.py:22-48).
    Read through ``s3dis.read_datasets``: no h5py is needed."""
    names = ["ply_data_train%d.h5" % i for i in range(5)] if train else ["ply_data_test%d.h5" % i for i in range(2)]
    parts = [_s3dis.read_datasets(os.path.join(path, n), ("data", "label")) for n in names]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


class ModelNet40:
    """``ModelNetDataLoader`` (ModelNetDataLoader.py:51-70) over the seven ``modelnet40_ply_hdf5_2048`` files, items prepared
    on the device.  ``augment`` is what the reference's augmentation branch intends and cannot run (see the module
    docstring): rotate, then jitter, draws in the order ``uniform()``, ``randn(1, 2048, 3)``."""
    class_names = class_names

    def __init__(self, path, train=True, device="cuda"):
        self.data, self.labels = load_modelnet(path, train)
        self.store = ShapeStore(self.data, None, self.labels.reshape(-1), device) if device is not None else None

    def __len__(self):
        return len(self.data)

    def batch(self, ids, augment=False, rng="numpy", out=None):
        """``(points [B, 2048, 3], label [B])`` on the device."""
        o, _, cls = prepare_shapes(self.store, ids, None, rotate=augment, jitter=augment, noise_cols=3, rng=rng, out=out)
        return o, cls


# ---- S3DIS --------------------------------------------------------------------------------------------------------------
class S3DISStore:
    """The blocks of ``s3dis.recognize_all_data`` (``data [n, 4096, 9]``, ``labels [n, 4096]``) resident on the device;
    ``batch`` is ``s3dis.S3DISDataLoader.__getitem__`` for a batch: all nine columns jittered, no rotation, no resampling."""

    def __init__(self, data, labels, device="cuda"):
        self.store = ShapeStore(np.asarray(data), labels, None, device)

    def __len__(self):
        return len(self.store)

    def batch(self, ids, augment=False, rng="numpy", out=None):
        """``(points [B, 4096, 9], labels [B, 4096])`` on the device."""
        o, lab, _ = prepare_shapes(self.store, ids, None, jitter=augment, noise_cols=self.store.C, rng=rng, out=out)
        return o, lab
