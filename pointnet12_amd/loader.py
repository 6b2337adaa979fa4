"""Per-batch cloud preparation on the HIP library.

The reference prepares every training item on the host (``SemKITTI_Loader.__getitem__``,
data_utils/SemKITTI_Loader.py:93-113): ``pcd_normalize`` (:23-30), ``pcd_jitter`` (:17-21, training only), then
``np.random.choice(length, npoints, replace=True)`` and two fancy-index gathers (:110-113); the collated batch is
copied to the GPU and transposed (semseg.py:131).  Here the raw scans stay resident in HBM (``ScanStore``: all of
SemanticKITTI's training split is ~25 GB, 288 GB are available) and one ``pn2_prepare_clouds`` launch writes the
``[B, N, 4]`` batch and its ``[B, N]`` labels; only the random draws cross the host boundary.

Two sources for the draws:
  * ``rng="numpy"`` (default): numpy's global generator in the reference's order -- per cloud ``randn(M, 4)`` (when
    training) then ``choice(M, npoints)`` -- so ``np.random.seed(s)`` reproduces the reference's batches bit for
    bit (a ``num_workers=0`` loader; worker processes reseed numpy in the reference as well).
  * ``rng=torch.Generator(device)``: draws on the device (same distributions, different stream): nothing but the
    scan numbers crosses PCIe.
"""
import numpy as np
import torch

from . import _lib

_p = _lib.ptr


class ScanStore:
    """Raw scans ``[M_i, 4]`` fp32 (x, y, z, intensity -- the .bin rows of kitti_utils.py:200) and their int32
    per-point classes, uploaded once and kept back to back in HBM."""

    def __init__(self, scans, labels=None, device="cuda"):
        if not scans:
            raise ValueError("ScanStore: no scans")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.Pn2Error("ScanStore: the HIP device is the only implementation")
        counts = [int(s.shape[0]) for s in scans]
        for s in scans:
            if s.ndim != 2 or s.shape[1] != 4:
                raise ValueError("ScanStore: scans must be [M, 4] (x, y, z, intensity)")
        self.row_count = torch.tensor(counts, dtype=torch.int64)
        self.row_begin = torch.cumsum(self.row_count, 0) - self.row_count
        self.raw = torch.from_numpy(np.ascontiguousarray(np.concatenate(scans, 0), np.float32)).to(self.device)
        self.label = None
        if labels is not None:
            if [int(l.shape[0]) for l in labels] != counts:
                raise ValueError("Scan and Label don't contain same number of points")     # kitti_utils.py:211
            self.label = torch.from_numpy(np.ascontiguousarray(np.concatenate(labels, 0), np.int32)).to(self.device)
        self._begin_dev = self.row_begin.to(self.device)
        self._count_dev = self.row_count.to(self.device)

    @classmethod
    def from_device(cls, raw, label, row_count):
        """A store over rows that are on the device already (``kitti.load_scans(ingest="device")``): ``raw`` float32 ``[rows, 4]``,
        ``label`` int32 ``[rows]`` or None, ``row_count`` the scans' row counts (host)."""
        self = cls.__new__(cls)
        self.device = raw.device
        if self.device.type != "cuda":
            raise _lib.Pn2Error("ScanStore: the HIP device is the only implementation")
        self.row_count = torch.as_tensor(np.asarray(row_count), dtype=torch.int64)
        if self.row_count.numel() == 0:
            raise ValueError("ScanStore: no scans")
        if raw.dim() != 2 or raw.shape[1] != 4 or raw.dtype != torch.float32 or int(self.row_count.sum()) != raw.shape[0] or \
                (label is not None and (label.dtype != torch.int32 or label.shape != (raw.shape[0],))):
            raise ValueError("ScanStore: raw must be float32 [sum(row_count), 4] and label int32 [sum(row_count)]")
        self.row_begin = torch.cumsum(self.row_count, 0) - self.row_count
        self.raw = raw.contiguous()
        self.label = None if label is None else label.contiguous()
        self._begin_dev = self.row_begin.to(self.device)
        self._count_dev = self.row_count.to(self.device)
        return self

    def __len__(self):
        return self.row_count.numel()


def pcd_jitter_noise(M, C=4, sigma=0.01, clip=0.05):
    """The clipped jitter rows of ``pcd_jitter`` (SemKITTI_Loader.py:17-19), from numpy's global generator."""
    return np.clip(sigma * np.random.randn(M, C), -1 * clip, clip).astype(np.float32)


def prepare_batch(store, scan_ids, npoints, train=True, rng="numpy", sigma=0.01, clip=0.05, out=None):
    """Batch of ``len(scan_ids)`` clouds: ``(points [B, npoints, 4] fp32, labels [B, npoints] int64 | None)`` on the
    device.  ``points.transpose(2, 1)`` is the ``[B, 4, N]`` tensor semseg.py:131 feeds the network.  ``out``: a
    ``(points, labels)`` pair of contiguous tensors to write into (the static inputs of a captured step)."""
    lib, st = _lib.load(), _lib.stream()
    ids = torch.as_tensor(scan_ids, dtype=torch.int64)
    B = ids.numel()
    if B == 0:
        raise ValueError("prepare_batch: empty batch")
    counts = store.row_count[ids]
    dev = store.device
    noise = noise_begin = None
    if rng == "numpy":
        rows, picks = [], []
        for m in counts.tolist():
            if train:
                rows.append(pcd_jitter_noise(m, 4, sigma, clip))
            picks.append(np.random.choice(m, npoints, replace=True))
        choice = torch.from_numpy(np.stack(picks).astype(np.int64)).to(dev)
        if train:
            noise = torch.from_numpy(np.concatenate(rows, 0)).to(dev)
            noise_begin = (torch.cumsum(counts, 0) - counts).to(dev)
    elif isinstance(rng, torch.Generator):
        cnt = counts.to(dev)
        u = torch.rand(B, npoints, device=dev, dtype=torch.float64, generator=rng)
        choice = torch.minimum((u * cnt[:, None]).long(), cnt[:, None] - 1)
        if train:
            total = int(counts.sum())
            noise = torch.randn(total, 4, device=dev, generator=rng).mul_(sigma).clamp_(-clip, clip)
            noise_begin = (torch.cumsum(counts, 0) - counts).to(dev)
    else:
        raise ValueError('prepare_batch: rng must be "numpy" or a device torch.Generator')
    ids_dev = ids.to(dev)
    begin, count = store._begin_dev[ids_dev], store._count_dev[ids_dev]
    if out is not None:
        points, labels = out
        if points.shape != (B, npoints, 4) or points.dtype != torch.float32 or not points.is_contiguous() or \
                (labels is not None and (labels.shape != (B, npoints) or labels.dtype != torch.int64
                                         or not labels.is_contiguous())):
            raise ValueError("prepare_batch: out must be contiguous ([B, npoints, 4] float32, [B, npoints] int64)")
        if labels is not None and store.label is None:
            raise ValueError("prepare_batch: the store holds no labels")
    else:
        points = torch.empty(B, npoints, 4, device=dev, dtype=torch.float32)
        labels = torch.empty(B, npoints, device=dev, dtype=torch.int64) if store.label is not None else None
    _lib.check(lib.pn2_prepare_clouds(_p(store.raw), _p(begin), _p(count), _p(store.label), _p(noise), _p(noise_begin),
                                      _p(choice), B, npoints, _p(points), _p(labels), None, st), "pn2_prepare_clouds")
    if out is not None:
        from . import pointnet_util as _U
        _U.bump_data_generation()             # a static buffer was refilled through a raw pointer: views of it are stale
    return points, labels


# --------------------------------------------------------------------------------------------------- the colour-generation task
class ColorStore:
    """The store of the colour-generation task (``ColorGeneratorLoader.get_data``, data_utils/ColorGenerator_Loader.py:54-80, which
    keeps ``[M, 7]`` rows x, y, z, i, c0, c1, c2 per scan in a cache): here one HBM allocation holds the raw ``[rows, 4]`` buffer
    and the colour ``[rows, 3]`` buffer back to back (``raw`` / ``color``: the layouts ``pn2_prepare_clouds`` and
    ``pn2_prepare_shapes`` read), plus ``valid`` bool ``[rows]`` (the point was inside the camera frame; outside it the colour is
    three zeros, as in the reference, which trains on those rows too)."""

    def __init__(self, row_count, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.Pn2Error("ColorStore: the HIP device is the only implementation")
        self.row_count = torch.as_tensor(np.asarray(row_count), dtype=torch.int64).reshape(-1)
        if self.row_count.numel() == 0:
            raise ValueError("ColorStore: no scans")
        self.row_begin = torch.cumsum(self.row_count, 0) - self.row_count
        rows = int(self.row_count.sum())
        self.buffer = torch.zeros(rows * 7, device=self.device, dtype=torch.float32)
        self.raw = self.buffer[:rows * 4].view(rows, 4)
        self.color = self.buffer[rows * 4:].view(rows, 3)
        self.valid = torch.zeros(rows, device=self.device, dtype=torch.bool)
        self._begin_dev = self.row_begin.to(self.device)
        self._count_dev = self.row_count.to(self.device)

    def __len__(self):
        return self.row_count.numel()

    @classmethod
    def from_scans(cls, scans, images, calib, mode="hsv", normalize=True, channel_order="rgb", device="cuda", chunk_rows=1 << 22):
        """``scans``: host arrays ``[M_i, 4]`` (x, y, z, intensity, already filtered to the camera's view: ``sample_image`` has no
        depth test); ``images``: one uint8 ``[H, W, 3]`` host array per scan; ``calib``: a ``kitti_view.Calibration``.  The
        scans are uploaded in chunks of about ``chunk_rows`` rows, as ``kitti.load_scans`` does, and every chunk is painted by ONE
        batched ``kitti_view.paint_points`` call (project + sample; a chunk ends early where the image size changes).  ``mode``,
        ``normalize``, ``channel_order``: ``sample_image``'s; the defaults store the reference's target, HSV in [0, 1]."""
        from . import kitti_view as KV
        scans, images = list(scans), list(images)
        if len(scans) != len(images):
            raise ValueError("ColorStore: one image per scan")
        for s in scans:
            if s.ndim != 2 or s.shape[1] != 4:
                raise ValueError("ColorStore: scans must be [M, 4] (x, y, z, intensity)")
        self = cls([int(s.shape[0]) for s in scans], device)
        dev = self.device
        at = k = 0
        while k < len(scans):
            j, rows = k, 0
            while j < len(scans) and (j == k or (rows < chunk_rows and images[j].shape == images[k].shape)):
                rows += int(scans[j].shape[0])
                j += 1
            if rows > 0:
                counts = self.row_count[k:j]
                raw = self.raw[at:at + rows]
                raw.copy_(torch.from_numpy(np.ascontiguousarray(np.concatenate(scans[k:j], 0), np.float32)))
                img = torch.from_numpy(np.ascontiguousarray(np.stack(images[k:j]), np.uint8)).to(dev)
                painted, valid = KV.paint_points(raw, calib, img, mode, normalize, channel_order,
                                                 row_begin=(torch.cumsum(counts, 0) - counts).to(dev), row_count=counts.to(dev),
                                                 max_rows=int(counts.max()), return_valid=True)
                self.color[at:at + rows] = painted[:, 4:]
                self.valid[at:at + rows] = valid
            at, k = at + rows, j
        return self


def color_window_start(length, npoints):
    """The crop's first row as ``ColorGeneratorLoader.__getitem__`` draws it (ColorGenerator_Loader.py:92-93):
    ``np.random.randint(0, length - npoints)`` for a longer cloud (the high end is exclusive, so the LAST window is never drawn, and
    a cloud one row longer always starts at 0), no draw and 0 otherwise."""
    return int(np.random.randint(0, length - npoints)) if length > npoints else 0


def prepare_color_batch(store, ids, npoints, train=True, rng="numpy", sigma=0.01, clip=0.05, out=None, return_valid=False):
    """``(points [B, npoints, 4], target [B, npoints, 3])`` float32 on the device: ``ColorGeneratorLoader.__getitem__``
    (ColorGenerator_Loader.py:82-101) for a batch over a ``ColorStore`` -- ``pcd_normalize``, the jitter when training, then the
    WINDOW: row ``i`` of the item is row ``(start + i) % length`` of the cloud.  For a cloud longer than ``npoints`` that is the crop
    ``[start, start + npoints)``; for ``length == npoints`` the cloud itself; a shorter cloud wraps, which is the reference's
    ``concatenate(pcd, pcd[0:short])`` GENERALISED to clouds shorter than half the window, where the reference returns a short
    item and fails at collate.  The window is computed on the device from ``start`` and the device-side counts; the points go
    through ``pn2_prepare_clouds`` and the targets through ``pn2_prepare_shapes`` with ``C = 3``, two launches.

    ``rng="numpy"``: numpy's global generator in the reference's order, per cloud ``randn(M, 4)`` (when training) and then
    ``randint(0, length - npoints)`` (a longer cloud only): ``np.random.seed(s)`` reproduces a ``num_workers=0`` loader bit for bit.
    A device ``torch.Generator``: the same distributions drawn on the device (``start = min((u * (length - npoints)).long(),
    length - npoints - 1)``, 0 where the cloud is not longer).  ``out``: a ``(points, target)`` pair of contiguous tensors.
    ``return_valid``: also bool ``[B, npoints]``, ``store.valid`` of the same rows (the point was inside the camera frame: the
    reference trains on the zero targets outside it as well; a loss over the valid rows alone needs this mask)."""
    lib, st = _lib.load(), _lib.stream()
    ids = torch.as_tensor(ids, dtype=torch.int64).reshape(-1)
    B, npoints = ids.numel(), int(npoints)
    if B == 0 or npoints < 1:
        raise ValueError("prepare_color_batch: empty batch")
    counts = store.row_count[ids]
    if int(counts.min()) < 1:
        raise ValueError("prepare_color_batch: an empty cloud has no window")
    dev = store.device
    noise = noise_begin = None
    if isinstance(rng, str) and rng == "numpy":
        rows, starts = [], []
        for m in counts.tolist():
            if train:
                rows.append(pcd_jitter_noise(m, 4, sigma, clip))
            starts.append(color_window_start(m, npoints))
        start = torch.tensor(starts, dtype=torch.int64).to(dev)
        if train:
            noise = torch.from_numpy(np.concatenate(rows, 0)).to(dev)
    elif isinstance(rng, torch.Generator):
        if train:
            noise = torch.randn(int(counts.sum()), 4, device=dev, generator=rng).mul_(sigma).clamp_(-clip, clip)
        span = (counts - npoints).to(dev)
        u = torch.rand(B, device=dev, dtype=torch.float64, generator=rng)
        start = torch.minimum((u * span).long(), span - 1).clamp_(min=0)
    else:
        raise ValueError('prepare_color_batch: rng must be "numpy" or a device torch.Generator')
    if train:
        noise_begin = (torch.cumsum(counts, 0) - counts).to(dev)
    ids_dev = ids.to(dev)
    begin, count = store._begin_dev[ids_dev], store._count_dev[ids_dev]
    choice = torch.remainder(start[:, None] + torch.arange(npoints, device=dev, dtype=torch.int64)[None, :], count[:, None]).contiguous()
    if out is not None:
        points, target = out
        if points.shape != (B, npoints, 4) or points.dtype != torch.float32 or not points.is_contiguous() or \
                target.shape != (B, npoints, 3) or target.dtype != torch.float32 or not target.is_contiguous():
            raise ValueError("prepare_color_batch: out must be contiguous ([B, npoints, 4] float32, [B, npoints, 3] float32)")
    else:
        points = torch.empty(B, npoints, 4, device=dev, dtype=torch.float32)
        target = torch.empty(B, npoints, 3, device=dev, dtype=torch.float32)
    _lib.check(lib.pn2_prepare_clouds(_p(store.raw), _p(begin), _p(count), None, _p(noise), _p(noise_begin), _p(choice), B, npoints,
                                      _p(points), None, None, st), "pn2_prepare_clouds")
    _lib.check(lib.pn2_prepare_shapes(_p(store.color), 3, _p(begin), _p(count), None, None, None, 0, None, _p(choice), B, npoints,
                                      _p(target), None, None, st), "pn2_prepare_shapes")
    if out is not None:
        from . import pointnet_util as _U
        _U.bump_data_generation()             # static buffers were refilled through raw pointers: views of them are stale
    if return_valid:
        return points, target, store.valid[begin[:, None] + choice]
    return points, target
