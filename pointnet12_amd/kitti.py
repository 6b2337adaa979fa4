"""SemanticKITTI scans from disk into the resident scan store.

Host-side parsing of the two per-scan files the reference trains on -- ``velodyne/%06d.bin`` (float32 x, y, z,
intensity) and ``labels/%06d.label`` (uint32: semantic class in the low 16 bits, instance id above) -- restating
``Semantic_KITTI_Utils.get`` (data_utils/kitti_utils.py:183-227): map the raw class through ``learning_map``, drop
the points of class 0 and shift the rest down by one (:215-221), and for the ``inview`` subset keep the camera's
field of view (:223-227 with ``points_basic_filter`` :259-280).  This runs once per scan when the store is filled;
everything per batch happens on the device (loader.prepare_batch).

``ScanFilter`` / ``read_scan_device`` / ``load_scans(ingest="device")`` do the same five steps on the device
(``pn2_scan_filter``, csrc/scan.hip): the raw ``.bin`` / ``.label`` words are uploaded as they are, and the kept rows,
their classes, their row numbers and the kept COUNT stay in device memory, so a frame path or a live feed needs no host
pass.  ``inverse_label_lut`` / ``write_labels`` go the other way: predicted training classes back to the dataset's raw
ids, and those into a ``.label`` file (``kitti_view.FrameSegmenter.label_scan`` produces them for every row of a scan).
The device rule is the one of include/pn2.h; it differs from ``in_view`` in one place only: the two angles are
fp64 ``atan2`` values rounded to float32, where numpy's float32 ``arctan2`` is a few ulp off the correctly rounded value
(and differs between numpy builds), so a point within a few float32 steps of a field-of-view border may fall on the
other side (tests/scan_filter_ref.py quantifies it).

The filter keeps the reference's exact forms: the azimuth test is ``-40 deg < atan2(y, x) < 40 deg`` on float32
angles, and the elevation test takes ``atan2(z, d)`` with d the full 3-D range ``sqrt(x^2 + y^2 + z^2)`` (not the
ground range), bounds -20 deg .. 20 deg (:263-268, :237-249).
"""
import ctypes

import numpy as np
import torch

from . import _lib, loader


def in_view(points, h_fov=(-40, 40), v_fov=(-20, 20)):
    """Boolean mask of the points inside the horizontal / vertical field of view (kitti_utils.py:259-280; the box
    limits of :251-257 are +-10 000 m, i.e. never active, and are kept for NaN parity: a NaN coordinate fails them)."""
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    d = np.sqrt(x ** 2 + y ** 2 + z ** 2)
    az = np.arctan2(y, x)
    el = np.arctan2(z, d)
    keep = np.logical_and(az > (-h_fov[1] * np.pi / 180), az < (-h_fov[0] * np.pi / 180))
    keep = np.logical_and(keep, np.logical_and(el < (v_fov[1] * np.pi / 180), el > (v_fov[0] * np.pi / 180)))
    lim = 10000
    box = np.logical_and.reduce((x > -lim, x < lim, y > -lim, y < lim, z > -lim, z < lim, d > -lim, d < lim))
    return np.logical_and(keep, box)


def read_scan(fn_velo, fn_label, learning_map, subset="all"):
    """One scan: ``(points [M, 4] float32, labels [M] int32 in 0..num_classes-1)`` as ``Semantic_KITTI_Utils.get``
    returns them.  ``learning_map``: dict raw class -> training class (0 = ignored), the ``learning_map`` block of
    the dataset's ``semantic-kitti.yaml``."""
    if subset not in ("all", "inview"):
        raise AssertionError(subset)
    points = np.fromfile(fn_velo, dtype=np.float32).reshape(-1, 4)
    raw = np.fromfile(fn_label, dtype=np.uint32).reshape(-1)
    if raw.shape[0] != points.shape[0]:
        raise ValueError("Scan and Label don't contain same number of points")
    sem = raw & 0xFFFF
    lut = np.full(int(max(max(learning_map), int(sem.max()) if sem.size else 0)) + 1, -1, np.int64)
    for k, v in learning_map.items():
        lut[int(k)] = int(v)
    label = lut[sem]
    if (label < 0).any():
        raise KeyError(int(sem[label < 0][0]))                  # a raw class missing from the map (dict lookup raises)
    label = label.astype(np.int32)
    keep = label != 0                                            # drop class 0, shift the others down (:218-221)
    points, label = points[keep], label[keep] - 1
    if subset == "inview":
        m = in_view(points)
        points, label = points[m], label[m]
    return points, label


def read_poses(fn_poses, Tr=None):
    """The dataset's ``poses.txt`` (one line per frame: the 12 numbers of a 3 x 4 ``[R | t]``, row-major, frame -> the sequence's
    first CAMERA frame) -> float64 [F,4,4].  With the calibration's ``Tr`` (velodyne -> camera, 12 numbers, [3,4] or [4,4]) the
    poses are returned in the SCANNER's frame, ``inv(Tr) @ P @ Tr``: ``inv(pose[i]) @ pose[j]`` is then what registering scan j to
    scan i (``registration.icp``) should find.  Host-side numpy."""
    rows = np.loadtxt(fn_poses, dtype=np.float64, ndmin=2)
    if rows.shape[1] != 12:
        raise ValueError("read_poses: every line must hold 12 numbers (got %d)" % rows.shape[1])
    poses = np.tile(np.eye(4), (rows.shape[0], 1, 1))
    poses[:, :3, :] = rows.reshape(-1, 3, 4)
    if Tr is None:
        return poses
    tr = np.eye(4)
    t = np.asarray(Tr, np.float64)
    tr[:3, :] = t.reshape(3, 4) if t.size == 12 else t.reshape(4, 4)[:3, :]
    return np.linalg.inv(tr) @ poses @ tr


def _read_files(fn_velo, fn_label):
    points = np.fromfile(fn_velo, dtype=np.float32).reshape(-1, 4)
    raw = None
    if fn_label is not None:
        raw = np.fromfile(fn_label, dtype=np.uint32).reshape(-1)
        if raw.shape[0] != points.shape[0]:
            raise ValueError("Scan and Label don't contain same number of points")
    return points, raw


class ScanBuffers:
    """The static buffers of one ``ScanFilter.filter`` call shape (``ScanFilter.buffers``): ``points`` float32 ``[rows, 4]``,
    ``labels`` / ``index`` int32 ``[rows]``, ``count`` int64 ``[B]`` and the kernel's ``workspace``."""

    def __init__(self, rows, B, max_rows, device):
        nbytes = _lib.workspace_bytes("pn2_scan_filter_workspace_bytes", (int(B), int(max_rows)), _lib.Pn2Error,
                                      "ScanBuffers: B = %d, max_rows = %d are not supported" % (B, max_rows))
        self.rows, self.B, self.max_rows = int(rows), int(B), int(max_rows)
        self.points = torch.empty(self.rows, 4, device=device, dtype=torch.float32)
        self.labels = torch.empty(self.rows, device=device, dtype=torch.int32)
        self.index = torch.empty(self.rows, device=device, dtype=torch.int32)
        self.count = torch.zeros(self.B, device=device, dtype=torch.int64)
        self.workspace = torch.empty(nbytes, device=device, dtype=torch.uint8)


class ScanFilter:
    """``Semantic_KITTI_Utils.get``'s class map, class drop, view filter and compaction on the device (``pn2_scan_filter``).

    ``learning_map``: dict raw class -> training class (0 = ignored), uploaded once as a look-up table; None serves
    unlabelled scans only.  The filter arguments have the defaults and the meaning of the reference's ``set_filter``
    (kitti_utils.py:229-235): ``subset="inview"`` takes ``h_fov = (-40, 40)``, ``v_fov = (-20, 20)`` where they are not given, as
    ``get`` does (:222), and every range defaults to ``(-10000, 10000)``.  ``subset="all"`` applies no angular test (``h_fov`` /
    ``v_fov`` must be None), and the range box only if one of the four ranges is given: without any, every row passes, NaN
    rows included, as in ``get``.  The angular thresholds are computed as the reference computes them (``-h_fov[1] * np.pi / 180``
    and so on) and rounded to float32, which is what numpy compares a float32 array with.

    ``error_flag`` (device int32, cleared at the start of every ``filter``) collects ``_lib.SCAN_ERR_CLASS`` (a raw class
    outside the map: the reference raises ``KeyError``, here the row is dropped) and ``_lib.SCAN_ERR_ROWS`` (a ``row_count``
    above ``max_rows``: the rows beyond are ignored); ``check()`` reads it back and raises."""

    def __init__(self, learning_map=None, subset="inview", h_fov=None, v_fov=None, x_range=None, y_range=None, z_range=None,
                 d_range=None, device="cuda"):
        if subset not in ("all", "inview"):
            raise AssertionError(subset)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.Pn2Error("ScanFilter: the HIP device is the only implementation")
        self.subset = subset
        ranges = (x_range, y_range, z_range, d_range)
        if subset == "inview":
            h_fov = (-40, 40) if h_fov is None else h_fov
            v_fov = (-20, 20) if v_fov is None else v_fov
            self.fov = np.array([-h_fov[1] * np.pi / 180, -h_fov[0] * np.pi / 180, v_fov[0] * np.pi / 180, v_fov[1] * np.pi / 180],
                                np.float64).astype(np.float32)
        else:
            if h_fov is not None or v_fov is not None:
                raise ValueError('ScanFilter: subset="all" applies no angular test (h_fov and v_fov must be None)')
            self.fov = None
        self.box = None
        if subset == "inview" or any(r is not None for r in ranges):
            self.box = np.array([r if r is not None else (-10000, 10000) for r in ranges], np.float64).reshape(8).astype(np.float32)
        self.lut = None
        if learning_map is not None:
            lut = np.full(int(max(learning_map)) + 1, -1, np.int32)
            for k, v in learning_map.items():
                lut[int(k)] = int(v)
            self.lut = torch.from_numpy(lut).to(self.device)
        self.error_flag = torch.zeros(1, device=self.device, dtype=torch.int32)
        self._zero = torch.zeros(1, device=self.device, dtype=torch.int64)

    def buffers(self, rows, B=1, max_rows=None):
        """``ScanBuffers`` for calls of ``B`` scans of at most ``max_rows`` rows each (default ``rows``) whose outputs fit ``rows``."""
        return ScanBuffers(rows, B, rows if max_rows is None else max_rows, self.device)

    def filter(self, raw, raw_label=None, row_begin=None, row_count=None, max_rows=None, out=None, out_begin=None):
        """``(points, labels, index, count)`` as device tensors.  ``raw``: float32 ``[rows, 4]`` on the device, the ``.bin`` rows of
        one scan or of B scans back to back; ``raw_label``: their ``.label`` words (32-bit: int32 or uint32 tensor ``[rows]``) or
        None for unlabelled scans (``labels`` is then None).  ``row_begin`` / ``row_count``: int64 ``[B]`` DEVICE tensors as
        ``pn2_prepare_clouds`` reads them (None: one scan, all of ``raw``); ``max_rows``: a host bound of every count (None:
        ``raw``'s rows).  Scan b's kept rows are ``points[out_begin[b] : out_begin[b] + count[b]]`` (``out_begin``: int64 ``[B]`` on
        the device, None: ``row_begin``) in scan order -- the reference's ``points[mask]`` -- with ``labels`` int32 (the class
        after the shift) and ``index`` int32 (the raw row inside its scan, strictly increasing) beside them; rows outside those
        ranges are not written.  ``count`` is int64 ``[B]`` and stays on the device: nothing is read back.  With ``out`` (a
        ``ScanBuffers`` of this shape) and ``row_begin`` / ``row_count`` given the call allocates nothing and can be captured
        in a graph; a captured call stays valid when ``row_count``'s content changes."""
        if not isinstance(raw, torch.Tensor) or not raw.is_cuda:
            raise _lib.Pn2Error("ScanFilter.filter: raw must live on the GPU: this package has no CPU path")
        if raw.dtype != torch.float32 or raw.dim() != 2 or raw.shape[1] != 4 or not raw.is_contiguous():
            raise ValueError("ScanFilter.filter: raw must be a contiguous float32 [rows, 4] tensor")
        rows = int(raw.shape[0])
        if raw_label is not None:
            if self.lut is None:
                raise ValueError("ScanFilter.filter: labels given, but the filter has no learning_map")
            if not raw_label.is_cuda or raw_label.element_size() != 4 or raw_label.is_floating_point() or \
                    raw_label.numel() != rows or not raw_label.is_contiguous():
                raise ValueError("Scan and Label don't contain same number of points")     # (or not 32-bit words on the device)
        if (row_begin is None) != (row_count is None):
            raise ValueError("ScanFilter.filter: row_begin and row_count go together")
        if row_begin is None:
            row_begin, row_count = self._zero, torch.full((1,), rows, device=self.device, dtype=torch.int64)
        B = int(row_begin.numel())
        for t in (row_begin, row_count) + (() if out_begin is None else (out_begin,)):
            if not t.is_cuda or t.dtype != torch.int64 or t.numel() != B or not t.is_contiguous():
                raise ValueError("ScanFilter.filter: row_begin, row_count and out_begin must be int64 [B] device tensors")
        max_rows = rows if max_rows is None else int(max_rows)
        if out is None:
            out = ScanBuffers(rows, B, max_rows, self.device)
        elif out.B != B or out.max_rows < max_rows:
            raise ValueError("ScanFilter.filter: out was made for B = %d, max_rows = %d" % (out.B, out.max_rows))
        p = _lib.ptr
        fp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        self.error_flag.zero_()                                      # an async fill, nothing is read back
        # (max_rows as the buffers were made for: the workspace layout follows it)
        _lib.check(_lib.load().pn2_scan_filter(p(raw), p(raw_label), p(row_begin), p(row_count), B, out.max_rows, p(self.lut),
                                               0 if self.lut is None else int(self.lut.numel()), fp(self.fov), fp(self.box),
                                               p(row_begin if out_begin is None else out_begin), p(out.points),
                                               p(out.labels) if raw_label is not None else None, p(out.index), p(out.count),
                                               p(self.error_flag), p(out.workspace), _lib.stream()), "pn2_scan_filter")
        return out.points, (out.labels if raw_label is not None else None), out.index, out.count

    def check(self):
        """Reads ``error_flag`` back: ``KeyError`` for a raw class missing from the map (as the reference's dict lookup),
        ``ValueError`` for a ``row_count`` above ``max_rows``."""
        flag = int(self.error_flag.item())
        if flag & _lib.SCAN_ERR_CLASS:
            raise KeyError("a raw class is missing from the learning map")
        if flag & _lib.SCAN_ERR_ROWS:
            raise ValueError("ScanFilter: a row_count is above max_rows")


def inverse_label_lut(learning_map_inv, device="cuda"):
    """int32 device table ``lut[c] = learning_map_inv[c + 1]`` for the training classes ``c = 0 .. K-1`` the network predicts:
    ``Semantic_KITTI_Utils.get`` drops training class 0 and shifts the others down by one (kitti_utils.py:215-219), and this
    undoes both -- predicted class ``c`` is the dataset's raw id ``learning_map_inv[c + 1]``.  ``learning_map_inv``: the block of
    that name of the dataset's ``semantic-kitti.yaml`` (training class -> raw id; its entry 0 is "unlabeled")."""
    inv = {int(k): int(v) for k, v in learning_map_inv.items()}
    ids = sorted(i for i in inv if i != 0)
    if not ids or ids != list(range(1, len(ids) + 1)):
        raise ValueError("learning_map_inv must name the training classes 1..K")
    if any(not 0 <= inv[i] <= 0xFFFF for i in ids):
        raise ValueError("learning_map_inv: a raw id does not fit the 16 semantic bits of a .label word")
    return torch.from_numpy(np.array([inv[i] for i in ids], np.int32)).to(torch.device(device))


def write_labels(fn, labels, instances=None):
    """Write per-point semantic ids in the dataset's ``.label`` format: one little-endian uint32 word per point, the semantic
    id in the low 16 bits and the instance id in the high 16 (``np.fromfile(fn, np.uint32) & 0xFFFF`` gives the semantic ids back,
    ``>> 16`` the instances).  ``labels``: an integer array or tensor (either side) of raw ids in 0 .. 65535; ``instances``: None
    (instance 0 everywhere) or as many integers in 0 .. 65535, e.g. ``label_scan(..., instances=)``'s ``scan_instances``.  A device
    tensor is read back here."""
    def host(values, what):
        if isinstance(values, torch.Tensor):
            values = values.detach().cpu().numpy()
        ids = np.asarray(values).reshape(-1)
        if ids.dtype.kind not in "iu":
            raise ValueError("write_labels: %s must be integers (got %s)" % (what, ids.dtype))
        return ids

    ids = host(labels, "labels")
    if ids.size and (int(ids.min()) < 0 or int(ids.max()) > 0xFFFF):
        raise ValueError("write_labels: a semantic id lies outside 0 .. 65535")
    words = ids.astype("<u4")
    if instances is not None:
        inst = host(instances, "instances")
        if inst.size != ids.size:
            raise ValueError("write_labels: %d instances for %d labels" % (inst.size, ids.size))
        if inst.size and (int(inst.min()) < 0 or int(inst.max()) > 0xFFFF):
            raise ValueError("write_labels: an instance id lies outside 0 .. 65535")
        words = (inst.astype("<u4") << np.uint32(16)) | words
    words.astype("<u4").tofile(fn)


def split_label_words(words, device=None):
    """``.label`` words -> ``(semantic, instance)`` int32 tensors on ``device``: the low and the high 16 bits, the inverse of what
    ``write_labels`` packs.  ``words``: a uint32 (or int32: the same bits) array or tensor of any shape; ``device`` None: a tensor's
    own device, the GPU for an array.  A few elementwise device operations, nothing is read back."""
    if isinstance(words, torch.Tensor):
        if words.element_size() != 4 or words.is_floating_point():
            raise ValueError("split_label_words: the words must be 32-bit integers (got %s)" % words.dtype)
        w = words.reshape(-1).contiguous().view(torch.int32)
        w = w if device is None else w.to(device)
    else:
        arr = np.ascontiguousarray(words).reshape(-1)
        if arr.dtype.kind not in "iu" or arr.dtype.itemsize != 4:
            raise ValueError("split_label_words: the words must be 32-bit integers (got %s)" % arr.dtype)
        w = _upload_words(arr, "cuda" if device is None else device)
    return w & 0xFFFF, (w >> 16) & 0xFFFF                                # (an arithmetic shift: the mask drops the copies of the sign)


def _upload_words(words, device):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(device)     # the same 32 bits (torch has no uint32 math)


def read_scan_device(fn_velo, fn_label, scan_filter):
    """``read_scan`` through the device: ``np.fromfile`` of both files, one upload, ``scan_filter.filter``.  Returns
    ``(points [M, 4] float32, labels [M] int32)`` as DEVICE tensors of exact size, for which the one kept count is read back
    (``ScanFilter.filter`` itself reads nothing back).  ``fn_label`` None: an unlabelled scan, ``labels`` is None.  A raw class
    missing from the map raises ``KeyError``, as ``read_scan`` does."""
    points, words = _read_files(fn_velo, fn_label)
    raw = torch.from_numpy(points).to(scan_filter.device)
    lab = None if words is None else _upload_words(words, scan_filter.device)
    pts, labels, _, count = scan_filter.filter(raw, lab)
    m = int(count.item())
    scan_filter.check()
    return pts[:m], (None if labels is None else labels[:m])


def _ingest_chunk(chunk, scan_filter, voxel=None):
    """One batched launch over the scans of ``chunk`` ([(points, words)], host arrays): (points, labels, counts) packed.  With a
    ``voxel.VoxelGrid`` the kept rows of every scan go through one batched ``pn2_voxel_grid`` launch before the pack."""
    dev = scan_filter.device
    counts = np.array([p.shape[0] for p, _ in chunk], np.int64)
    begins = np.cumsum(counts) - counts
    if counts.sum() == 0:                                            # (nothing to launch on)
        return torch.empty(0, 4, device=dev), torch.empty(0, device=dev, dtype=torch.int32), np.zeros(len(chunk), np.int64)
    raw = torch.from_numpy(np.ascontiguousarray(np.concatenate([p for p, _ in chunk], 0))).to(dev)
    lab = _upload_words(np.concatenate([w for _, w in chunk], 0), dev)
    begin_dev = torch.from_numpy(begins).to(dev)
    pts, labels, _, kept = scan_filter.filter(raw, lab, begin_dev, torch.from_numpy(counts).to(dev), int(counts.max()))
    if voxel is not None:
        pts, labels, _, kept, _, _ = voxel.downsample(pts, labels, begin_dev, kept, int(counts.max()))
    kept = kept.cpu().numpy()                                        # the one read-back of the chunk
    scan_filter.check()
    if voxel is not None:
        voxel.check()
    total = int(kept.sum())
    out_p = torch.empty(total, 4, device=dev, dtype=torch.float32)
    out_l = torch.empty(total, device=dev, dtype=torch.int32)
    at = 0
    for b, k in zip(begins.tolist(), kept.tolist()):                 # the pack: device-to-device copies of the kept runs
        out_p[at:at + k] = pts[b:b + k]
        out_l[at:at + k] = labels[b:b + k]
        at += k
    return out_p, out_l, kept


def load_scans(pairs, learning_map, subset="inview", device="cuda", ingest="host", chunk_rows=1 << 22, voxel=None):
    """``ScanStore`` over the ``(bin_path, label_path)`` pairs (a sequence's scans, e.g. every second one for
    training as SemKITTI_Loader.py:62-66 selects them).  ``ingest="host"``: every scan through ``read_scan`` (numpy).
    ``ingest="device"``: the raw files are uploaded in chunks of about ``chunk_rows`` rows, each chunk goes through one
    batched ``pn2_scan_filter`` launch, its kept counts are read back once and the kept runs are packed into the store; the
    store equals the host one except where a point lies within a few float32 steps of a field-of-view border (module
    docstring).  ``voxel`` (a ``voxel.VoxelGrid``, ``ingest="device"`` only): every scan is downsampled to one row per occupied
    cell after the filter and before it enters the store (``pn2_voxel_grid``, one batched launch per chunk)."""
    if ingest not in ("host", "device"):
        raise ValueError('load_scans: ingest must be "host" or "device"')
    if voxel is not None and ingest != "device":
        raise ValueError('load_scans: a voxel grid needs ingest="device"')
    if ingest == "device":
        pairs = list(pairs)
        if not pairs:
            raise ValueError("ScanStore: no scans")
        scan_filter = ScanFilter(learning_map, subset, device=device)
        parts, chunk, rows = [], [], 0
        for k, (fn_velo, fn_label) in enumerate(pairs):
            chunk.append(_read_files(fn_velo, fn_label))
            rows += chunk[-1][0].shape[0]
            if rows >= chunk_rows or k == len(pairs) - 1:
                parts.append(_ingest_chunk(chunk, scan_filter, voxel))
                chunk, rows = [], 0
        return loader.ScanStore.from_device(torch.cat([p for p, _, _ in parts]), torch.cat([l for _, l, _ in parts]),
                                            np.concatenate([c for _, _, c in parts]))
    scans, labels = [], []
    for fn_velo, fn_label in pairs:
        p, l = read_scan(fn_velo, fn_label, learning_map, subset)
        scans.append(p)
        labels.append(l)
    return loader.ScanStore(scans, labels, device)
