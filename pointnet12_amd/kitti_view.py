"""The second half of the reference's KITTI demo (``python pcdvis.py``) on the device: labels, pixels, image.

``pcdvis.py:115-144`` reads a scan, resamples it to 25 000 points, normalises it, runs the network and takes the arg-max; it
then projects the points into the camera (``Semantic_KITTI_Utils.torch_project_3d_to_2d``), colours them by class and draws them
one ``cv2.circle`` at a time (``draw_2d_points``, data_utils/kitti_utils.py:368-379).  ``kitti.read_scan`` /
``loader.prepare_batch`` and the model zoo cover the first half; this module is the second, on ``csrc/view.hip``:

  * ``predict`` / ``merge_classes``   ``logits[0].argmax(-1)`` and the class merges of ``KITTI_2_Common`` /
    ``SemKITTI_2_Common`` (kitti_utils.py:41-58, :92-117) -- ``pn2_seg_predict``;
  * ``project_3d_to_2d``              kitti_utils.py:313-336 -- ``pn2_project_points``;
  * ``draw_2d_points`` / ``draw_2d_top_view``   kitti_utils.py:368-392 -- ``pn2_splat_discs`` + ``pn2_splat_resolve``;
  * ``render_points``                 the 3-D ego view, ``Window_Manager.update`` (pcdvis.py:31-51, :143): the scan through the fixed
    pinhole camera of ``config/ego_view.json`` (``PinholeCamera.from_json``), square points of ``config/render_option.json``'s
    size (``RenderOption.from_json``), nearest point per pixel -- ``pn2_depth_splat`` + ``pn2_depth_resolve`` +
    ``pn2_splat_resolve``; also the depth image and the index image (which point is visible where) of a cloud;
  * ``sample_image`` / ``paint_points`` / ``hsv_to_rgb``   the image -> points direction, on ``csrc/image.hip``: the colour of the pixel
    under each projected point (the per-point loop of data_utils/ColorGenerator_Loader.py:59-69), RGB or OpenCV-style 8-bit HSV,
    and the way back for looking at a prediction -- ``pn2_sample_image`` / ``pn2_hsv_to_rgb``;
  * ``FrameSegmenter``                the frame loop's body, device tensors in and out, nothing read back.

Nothing here copies the reference's tables: class names and colours come from the dataset's own ``semantic-kitti.yaml``
(``classes_from_config``: ``labels[learning_map_inv[i]]`` and ``color_map[learning_map_inv[i]]``, which is what the reference's
literal lists hold, entry for entry), merge lists come from the caller in the reference's ``'a+b'`` format.

Differences from the reference, all deliberate:

  * ``project_3d_to_2d`` (and its alias ``torch_project_3d_to_2d``) returns the numbers of the reference's NUMPY method
    (fp64 products on fp32 points, each stage stored as float32, fp32 division) bit for bit.  The reference's torch method, an
    fp32 ``bmm``, differs from those by rounding; it has no counterpart here.
  * Pixel coordinates are ``astype(np.int32)``'s truncation toward zero.  Where a projected coordinate is not finite or its
    magnitude is 2^31 or more, numpy's cast is undefined (it depends on the platform); here such a point gets ``INT32_MIN`` in
    both components and is never drawn.
  * Drawing order.  The reference draws point after point, so a pixel shows the last point that covered it; here every pixel
    takes the largest covering point index (an integer maximum), which is the same image, bit-identical from run to run.
  * THE DISC TABLES ARE UNVERIFIED AGAINST OPENCV.  ``cv2.circle(..., radius, color, -1)`` fills a rasterised disc; the two
    default tables below (radius 2: rows of 3, 5, 5, 5, 3 pixels = 21; radius 3: 3, 5, 7, 7, 7, 5, 3 = 37) were written from
    memory of OpenCV's filled-circle rasteriser and could not be checked, because OpenCV was not available where this was
    written.  The tests hold the kernel to the table, not to OpenCV.  Any other radius needs an explicit ``half_widths``.
  * THE EGO VIEW'S RASTERISATION RULE IS UNVERIFIED AGAINST OPEN3D.  The reference lets open3d's GL window draw the cloud;
    open3d was not available where this was written, so ``render_points`` states its rule itself (``pn2_depth_splat`` in
    include/pn2.h): an fp64 pinhole projection with the principal point counting pixel centres, OpenGL's rule for a
    non-antialiased point of integer size (a square of ``point_size`` pixels, ``floor`` of the window coordinate, plus a half for
    even sizes), and ``GL_LESS`` on the float32 camera depth with the lowest point index winning among equal depths.  The tests
    hold the kernel to an fp64 restatement of that rule, not to open3d; a pixel here and there may differ from open3d's window.
  * THE EGO VIEW'S NEAR / FAR PLANES ARE THIS PACKAGE'S CHOICE (0.1 and 1000 in the cloud's units), also unverified: open3d
    derives its clipping planes from the scene's bounding box.  Lighting, normals and the coordinate frame are not drawn.
  * THE HSV RULE IS UNVERIFIED AGAINST OPENCV.  ``sample_image(mode="hsv")`` states OpenCV's 8-bit ``COLOR_BGR2HSV`` as an integer
    rule written from memory of OpenCV's scalar code (include/pn2.h, ``pn2_sample_image``); OpenCV was not available where this
    was written.  The rule was checked against the real-valued definition over all 2^24 colours (hue within 0.640 of
    ``30 * sector``, saturation within 0.522 of ``255 d / v``); the tests hold the kernel to the rule, not to OpenCV.
    ``hsv_to_rgb`` is this package's own fp64 definition; OpenCV's float-based ``HSV2RGB`` is not claimed bit for bit.
  * ``sample_image`` has NO DEPTH TEST, as the reference has none: a point behind the camera that projects into the frame takes
    that pixel.  Filter first (``kitti.ScanFilter`` with the ``inview`` subset).  Its in-image test works on TRUNCATED pixel
    coordinates, as the reference's does: a projected coordinate in (-1, 0) has become 0 and counts as inside.
  * float32 log-probabilities on the GPU only: a CPU tensor raises ``Pn2Error``; there is no fallback path.
"""
import ctypes
import json
import math

import numpy as np
import torch

from . import _lib
from ._lib import check as _check, ptr as _p
from .metrics import MAX_CLASSES, _rows

INT32_MIN = -2 ** 31
MAX_GROUPS = 64
# row dy = j - radius of the disc covers dx in [-half_width[j], half_width[j]] -- see the module docstring: unverified against OpenCV
DISC_HALF_WIDTHS = {2: (1, 2, 2, 2, 1), 3: (1, 2, 3, 3, 3, 2, 1)}


# ------------------------------------------------------------------------------------------------------------- calibration
def _values(val):
    return np.array(val.split(), dtype=np.float64)


def calib_velo2cam(fn):
    """``(R [3, 3], T [3, 1])`` float64 of a KITTI ``calib_velo_to_cam.txt`` (kitti_utils.py:282-295)."""
    R = T = None
    with open(fn, "r") as f:
        for line in f:
            if ":" not in line:
                continue
            key, val = line.split(":", 1)
            if key == "R":
                R = _values(val).reshape(3, 3)
            if key == "T":
                T = _values(val).reshape(3, 1)
    if R is None or T is None:
        raise ValueError("%s holds no R / T line" % fn)
    return R, T


def calib_cam2cam(fn, mode="02"):
    """``P [3, 3]`` float64: the first three columns of ``P_rect_<mode>`` of a KITTI ``calib_cam_to_cam.txt`` (:297-311)."""
    P = None
    with open(fn, "r") as f:
        for line in f:
            if ":" not in line:
                continue
            key, val = line.split(":", 1)
            if key == ("P_rect_" + mode):
                P = _values(val).reshape(3, 4)[:3, :3]
    if P is None:
        raise ValueError("%s holds no P_rect_%s line" % (fn, mode))
    return P


class Calibration:
    """``R [3, 3]``, ``T [3, 1]``, ``P [3, 3]`` (float64) and ``RT = [R | T]`` (kitti_utils.py:148-150)."""

    def __init__(self, R, T, P):
        self.R = np.ascontiguousarray(R, np.float64).reshape(3, 3)
        self.T = np.ascontiguousarray(T, np.float64).reshape(3, 1)
        self.P = np.ascontiguousarray(P, np.float64).reshape(3, 3)
        self.RT = np.ascontiguousarray(np.concatenate((self.R, self.T), axis=1))

    @classmethod
    def from_files(cls, fn_velo2cam, fn_cam2cam, mode="02"):
        R, T = calib_velo2cam(fn_velo2cam)
        return cls(R, T, calib_cam2cam(fn_cam2cam, mode))


# ------------------------------------------------------------------------------------------------------- classes and merges
def classes_from_config(cfg):
    """``(class_names, colors uint8 [K, 3], colors_bgr uint8 [K, 3])`` of the training classes 1..K of a ``semantic-kitti.yaml``
    (a dict with its ``labels``, ``color_map`` and ``learning_map_inv`` blocks): training class ``i`` is entry ``i - 1``, named
    ``labels[learning_map_inv[i]]`` and coloured ``color_map[learning_map_inv[i]]`` -- the reference's ``sem_kitti_class_names``
    / ``sem_kitti_colors`` (kitti_utils.py:120-129); ``colors_bgr`` is each row reversed (:181)."""
    inv = {int(k): int(v) for k, v in cfg["learning_map_inv"].items()}
    labels = {int(k): v for k, v in cfg["labels"].items()}
    cmap = {int(k): v for k, v in cfg["color_map"].items()}
    ids = sorted(i for i in inv if i != 0)
    if ids != list(range(1, len(ids) + 1)):
        raise ValueError("learning_map_inv must name the training classes 1..K")
    names = [str(labels[inv[i]]) for i in ids]
    colors = np.array([list(cmap[inv[i]]) for i in ids], np.uint8).reshape(len(ids), 3)
    return names, colors, np.ascontiguousarray(colors[:, ::-1])


class Groups:
    """A merge table: group ``g`` consists of the classes ``member[begin[g]:begin[g + 1]]`` (int32 arrays, the layout
    ``pn2_seg_predict`` reads); ``names`` the merged names, ``first`` each group's first member, ``colors`` its colour."""

    def __init__(self, begin, member, names=None, colors=None):
        self.begin = np.ascontiguousarray(begin, np.int32)
        self.member = np.ascontiguousarray(member, np.int32)
        if self.begin.ndim != 1 or self.begin.size < 2 or self.begin[0] != 0 or (np.diff(self.begin) <= 0).any() or \
                self.begin[-1] != self.member.size:
            raise ValueError("Groups: begin must rise from 0 to len(member), no group empty")
        if len(self) > MAX_GROUPS:
            raise _lib.Pn2Error("Groups: %d groups are not supported (at most %d)" % (len(self), MAX_GROUPS))
        self.names = list(names) if names is not None else None
        self.first = self.member[self.begin[:-1]]
        self.colors = colors

    def __len__(self):
        return int(self.begin.size) - 1

    def members(self, g):
        return self.member[self.begin[g]:self.begin[g + 1]].tolist()


def merge_groups(class_names, merged, colors=None):
    """``Groups`` of a merge list in the reference's format, e.g. ``['road', 'parking+sidewalk', ...]``: the members of each entry
    are ``class_names.index`` of its ``'+'``-separated names (an unknown name raises ``ValueError``, as ``list.index`` does), in
    the order written; any number of members per group (the reference raises above two).  With ``colors`` ``[K, 3]``,
    ``.colors`` holds the colour of each group's FIRST member (kitti_utils.py:83-87)."""
    class_names = list(class_names)
    begin, member = [0], []
    for entry in merged:
        for name in entry.split("+"):
            member.append(class_names.index(name))
        begin.append(len(member))
    g = Groups(begin, member, merged)
    if colors is not None:
        g.colors = np.ascontiguousarray(np.asarray(colors)[g.first])
    return g


def _as_groups(groups):
    if groups is None or isinstance(groups, Groups):
        return groups
    begin, member = groups
    return Groups(begin, member)


# ------------------------------------------------------------------------------------------------------------------ predict
def _i32p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _logp(log_probs, what):
    if not isinstance(log_probs, torch.Tensor) or not log_probs.is_cuda:
        raise _lib.Pn2Error("%s: log_probs must live on the GPU: this package has no CPU path" % what)
    if log_probs.dtype != torch.float32:
        raise RuntimeError("%s: log_probs must be float32 (got %s)" % (what, log_probs.dtype))
    C = int(log_probs.shape[-1])
    if not 1 <= C <= MAX_CLASSES:
        raise _lib.Pn2Error("%s: %d classes are not supported (1 <= C <= %d; there is no fallback path)" % (what, C, MAX_CLASSES))
    logp, B, N, ld = _rows(log_probs.detach(), C)
    return logp, B * N, C, ld


def _seg_predict(logp, R, C, ld, groups, pred, merged):
    G = 0 if groups is None else len(groups)
    if groups is not None and (groups.member.min() < 0 or groups.member.max() >= C):
        raise ValueError("groups name class %d, log_probs has %d columns" % (int(groups.member.max()), C))
    if R > 0:
        _check(_lib.load().pn2_seg_predict(_p(logp), ld, R, C, _i32p(groups.begin) if G else None, _i32p(groups.member) if G else None,
                                           G, _p(pred), _p(merged), G, _lib.stream()), "pn2_seg_predict")


def predict(log_probs, groups=None, out=None):
    """int64 labels ``[...]`` of log-probabilities ``[B, N, C]`` or ``[R, C]``: ``log_probs.max(-1)[1]`` exactly (the lowest index
    on ties, the first NaN if there is one).  With ``groups`` (``merge_groups``) the arg-max is taken over the merged classes:
    ``merge_classes(log_probs, groups).max(-1)[1]`` without materialising them.  A column slice of a padded buffer is read in
    place.  Nothing is read back: the call can be captured in a graph (``out``: a contiguous int64 tensor to write into)."""
    groups = _as_groups(groups)
    logp, R, C, ld = _logp(log_probs, "predict")
    shape = tuple(log_probs.shape[:-1])
    if out is None:
        out = torch.empty(shape, device=logp.device, dtype=torch.int64)
    elif out.dtype != torch.int64 or out.device != logp.device or out.numel() != R or not out.is_contiguous():
        raise ValueError("predict: out must be a contiguous int64 tensor of %d elements on %s" % (R, logp.device))
    _seg_predict(logp, R, C, ld, groups, out, None)
    return out


def merge_classes(log_probs, groups):
    """``[..., C]`` -> ``[..., G]``: column ``g`` is the maximum over the members of group ``g`` (NaN where any member is NaN, as
    ``Tensor.max(dim)``) -- ``SemKITTI_2_Common.__call__`` (kitti_utils.py:92-117) for any number of members per group."""
    groups = _as_groups(groups)
    if groups is None:
        raise ValueError("merge_classes needs a group table (merge_groups)")
    logp, R, C, ld = _logp(log_probs, "merge_classes")
    out = torch.empty(tuple(log_probs.shape[:-1]) + (len(groups),), device=logp.device, dtype=torch.float32)
    _seg_predict(logp, R, C, ld, groups, None, out)
    return out


# ------------------------------------------------------------------------------------------------------------------ project
def _xyz_rows(pts, what):
    """[N, >= 3] float32 on the GPU -> (tensor, N, row pitch), rows read in place when their elements are adjacent."""
    if not isinstance(pts, torch.Tensor) or not pts.is_cuda:
        raise _lib.Pn2Error("%s: points must live on the GPU: this package has no CPU path" % what)
    if pts.dtype != torch.float32:
        raise RuntimeError("%s: points must be float32 (got %s)" % (what, pts.dtype))
    if pts.dim() != 2 or pts.shape[1] < 3:
        raise AssertionError(tuple(pts.shape))
    pts = pts.detach()
    N = int(pts.shape[0])
    if N > 1 and (pts.stride(1) != 1 or pts.stride(0) < 3 or pts.stride(0) >= 2 ** 31):
        pts = pts[:, :3].contiguous()
    elif N == 1 and pts.stride(1) != 1:
        pts = pts[:, :3].contiguous()
    return pts, N, int(pts.stride(0)) if N > 1 else 3


def project_3d_to_2d(pts_3d, calib, return_pixels=False, out=None):
    """``pts_2d`` float32 ``[N, 2]`` of velodyne points ``[N, 3]`` (or the first three columns of ``[N, 4]`` scan rows, read in
    place): ``Semantic_KITTI_Utils.project_3d_to_2d`` (kitti_utils.py:313-336), bit for bit.  These are the NUMPY method's
    numbers; the reference's ``torch_project_3d_to_2d`` (an fp32 ``bmm``) differs from them by rounding.

    ``return_pixels``: also int32 ``[N, 2]``, ``pts_2d.astype(np.int32)`` (truncation toward zero, :374).  A point whose
    projection is not finite (on the camera plane) or reaches 2^31 in magnitude gets ``INT32_MIN`` in both components: numpy's
    cast is undefined there, and the drawing kernels skip such points.  ``out``: ``(pts_2d | None, pix | None)`` buffers to write
    into (a given ``pix`` is filled either way); what is RETURNED depends on ``return_pixels`` alone."""
    pts, N, ld = _xyz_rows(pts_3d, "project_3d_to_2d")
    pts_2d, pix = out if out is not None else (None, None)
    if pts_2d is None:
        pts_2d = torch.empty(N, 2, device=pts.device, dtype=torch.float32)
    if pix is None and return_pixels:
        pix = torch.empty(N, 2, device=pts.device, dtype=torch.int32)
    if pts_2d.shape != (N, 2) or pts_2d.dtype != torch.float32 or not pts_2d.is_contiguous() or \
            (pix is not None and (pix.shape != (N, 2) or pix.dtype != torch.int32 or not pix.is_contiguous())):
        raise ValueError("project_3d_to_2d: out must be contiguous ([N, 2] float32, [N, 2] int32 | None)")
    if N > 0:
        _check(_lib.load().pn2_project_points(_p(pts), ld, N, calib.RT.ctypes.data_as(ctypes.c_void_p),
                                              calib.P.ctypes.data_as(ctypes.c_void_p), _p(pts_2d), _p(pix), _lib.stream()),
               "pn2_project_points")
    return (pts_2d, pix) if return_pixels else pts_2d


torch_project_3d_to_2d = project_3d_to_2d


def top_view_pixels(pcd_3d, out=None):
    """int32 ``[N, 2]`` disc centres ``(Y, X)`` of the top view (kitti_utils.py:387-390): ``X = int(-x*800 + 600)``,
    ``Y = int(-y*800 + 400)`` in Python's float arithmetic; ``INT32_MIN`` where Python's ``int()`` would raise or leave int32."""
    pts, N, ld = _xyz_rows(pcd_3d, "top_view_pixels")
    if out is None:
        out = torch.empty(N, 2, device=pts.device, dtype=torch.int32)
    elif out.shape != (N, 2) or out.dtype != torch.int32 or not out.is_contiguous():
        raise ValueError("top_view_pixels: out must be a contiguous [N, 2] int32 tensor")
    if N > 0:
        _check(_lib.load().pn2_project_points(_p(pts), ld, N, None, None, None, _p(out), _lib.stream()), "pn2_project_points")
    return out


def pcd_unnormalize(pcd):
    """The inverse of the loader's normalisation (``pcd_unnormalize``, data_utils/SemKITTI_Loader.py:32-38) on a tensor
    ``[N, 4]``: x*70, y*70, z*3, i/2 + 0.5 (one scaled copy; the offset goes to the intensity column alone, so a -0.0
    coordinate keeps its sign)."""
    out = pcd * pcd.new_tensor([70.0, 70.0, 3.0, 0.5])
    out[:, 3] += 0.5
    return out


# --------------------------------------------------------------------------------------------------------------------- draw
def _half_widths(radius, half_widths):
    radius = int(radius)
    if half_widths is None:
        if radius not in DISC_HALF_WIDTHS:
            raise ValueError("draw: no default disc table for radius %d (only %s): pass half_widths, %d row half-widths"
                             % (radius, sorted(DISC_HALF_WIDTHS), 2 * radius + 1))
        half_widths = DISC_HALF_WIDTHS[radius]
    hw = np.ascontiguousarray(half_widths, np.int32)
    if hw.shape != (2 * radius + 1,):
        raise ValueError("draw: half_widths must hold 2 * radius + 1 = %d rows" % (2 * radius + 1))
    return radius, hw


def to_pixels(pts_2d):
    """``pts_2d.astype(np.int32)`` of a float tensor ``[N, 2]`` under the rule of ``project_3d_to_2d``: truncation toward zero,
    ``INT32_MIN`` in both components of a point that is not finite or reaches 2^31."""
    ok = (torch.isfinite(pts_2d) & (pts_2d.abs() < 2.0 ** 31)).all(-1, keepdim=True)
    return torch.where(ok, pts_2d, torch.zeros_like(pts_2d)).trunc().to(torch.int32).masked_fill(~ok, INT32_MIN).contiguous()


def _dev_u8(a, device, what):
    if isinstance(a, torch.Tensor):
        if a.dtype != torch.uint8:
            raise RuntimeError("%s must be uint8 (got %s)" % (what, a.dtype))
        return a.to(device).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, np.uint8)).to(device)


def draw_2d_points(pts_2d, labels, colors, image=None, size=(375, 1242), radius=2, half_widths=None, out=None, owner=None,
                   err=None):
    """The image ``draw_2d_points`` paints (kitti_utils.py:368-379): uint8 ``[H, W, 3]`` on the device, pixel order
    ``[row = y, col = x]``.  ``pts_2d``: float ``[N, 2]`` ``(x, y)`` (cast as ``to_pixels`` does) or int32 ``[N, 2]`` pixel
    centres (``project_3d_to_2d(..., return_pixels=True)``).  Point ``i`` paints the disc of ``radius`` around its centre with
    ``colors[labels[i]]`` (``colors`` uint8 ``[C, 3]``, ``labels`` int64 ``[N]``), later points over earlier ones; ``image`` is the
    background (uint8 ``[H, W, 3]``, not modified; None: black, ``size = (H, W)``).  Default disc tables exist for radius 2 and 3
    only (see the module docstring: unverified against OpenCV); any other radius needs ``half_widths``.

    A label outside ``[0, C)`` paints nothing and sets ``err`` (a zeroed device int32 tensor).  Without ``err`` the flag is
    read back and raises ``IndexError`` (skipped under stream capture).  ``out`` / ``owner``: the image and a uint32-sized
    (int32) ``[H * W]`` scratch to write into; with both and ``err`` given the call allocates nothing."""
    if not isinstance(pts_2d, torch.Tensor) or not pts_2d.is_cuda or \
            (labels is not None and (not isinstance(labels, torch.Tensor) or not labels.is_cuda)):
        raise _lib.Pn2Error("draw_2d_points: points and labels must live on the GPU: this package has no CPU path")
    radius, hw = _half_widths(radius, half_widths)
    dev = pts_2d.device
    if pts_2d.dim() != 2 or pts_2d.shape[1] != 2:
        raise AssertionError(tuple(pts_2d.shape))
    N = int(pts_2d.shape[0])
    if labels is None:                                               # per-point colours: point i paints colors[i]
        if tuple(np.shape(colors)) != (N, 3):
            raise ValueError("draw_2d_points: without labels, colors must be uint8 [%d, 3], one row per point" % N)
        labels = torch.arange(N, device=dev, dtype=torch.int64)
    if labels.numel() != N or labels.dtype != torch.int64:
        raise ValueError("draw_2d_points: labels must be int64 [%d]" % N)
    pix = pts_2d.contiguous() if pts_2d.dtype == torch.int32 else to_pixels(pts_2d.detach())
    labels = labels.reshape(-1).contiguous()
    colors = _dev_u8(colors, dev, "colors")
    if colors.dim() != 2 or colors.shape[1] != 3:
        raise ValueError("draw_2d_points: colors must be [C, 3]")
    if image is not None:
        image = _dev_u8(image, dev, "image")
        if image.dim() != 3 or image.shape[2] != 3:
            raise ValueError("draw_2d_points: image must be [H, W, 3]")
        size = (int(image.shape[0]), int(image.shape[1]))
    H, W = int(size[0]), int(size[1])
    if out is None:
        out = torch.empty(H, W, 3, device=dev, dtype=torch.uint8)
    elif out.shape != (H, W, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != dev:
        raise ValueError("draw_2d_points: out must be a contiguous uint8 [%d, %d, 3] tensor on %s" % (H, W, dev))
    if owner is None:
        owner = torch.empty(H * W, device=dev, dtype=torch.int32)
    elif owner.numel() != H * W or owner.element_size() != 4 or not owner.is_contiguous() or owner.device != dev:
        raise ValueError("draw_2d_points: owner must be a contiguous 32-bit tensor of %d elements on %s" % (H * W, dev))
    flag = err if err is not None else torch.zeros(1, device=dev, dtype=torch.int32)
    lib, st = _lib.load(), _lib.stream()
    _check(lib.pn2_splat_discs(_p(pix), N, _i32p(hw), radius, H, W, _p(owner), st), "pn2_splat_discs")
    _check(lib.pn2_splat_resolve(_p(owner), H, W, _p(labels), N, _p(colors), int(colors.shape[0]), _p(image), _p(out), _p(flag), st),
           "pn2_splat_resolve")
    if err is None and not torch.cuda.is_current_stream_capturing() and int(flag.item()) != 0:
        raise IndexError("draw_2d_points: a label is outside [0, %d)" % colors.shape[0])
    return out


def draw_2d_top_view(pcd_3d, labels, colors, out=None, owner=None, err=None):
    """The 600 x 800 top view of ``draw_2d_top_view`` (kitti_utils.py:381-392) of NORMALISED points ``[N, >= 3]``: discs of radius
    3 at ``(Y, X)``, on black."""
    return draw_2d_points(top_view_pixels(pcd_3d), labels, colors, None, (600, 800), 3, None, out, owner, err)


# ------------------------------------------------------------------------------------------------------------ image -> points
_MODES = {"rgb": _lib.IMAGE_RGB, "hsv": _lib.IMAGE_HSV}
_ORDERS = {"rgb": _lib.CHANNELS_RGB, "bgr": _lib.CHANNELS_BGR}


def _code(table, key, what):
    if key not in table:
        raise ValueError("%s must be one of %s (got %r)" % (what, sorted(table), key))
    return table[key]


def _color_rows(out, M, dev, what, zero):
    """The ``out`` of ``sample_image``: float32 ``[M, 3]`` whose rows may be a column slice of wider rows -> (tensor, pitch)."""
    if out is None:
        out = (torch.zeros if zero else torch.empty)(M, 3, device=dev, dtype=torch.float32)
    elif not isinstance(out, torch.Tensor) or out.shape != (M, 3) or out.dtype != torch.float32 or out.device != dev or \
            (M > 0 and out.stride(1) != 1) or (M > 1 and not 3 <= out.stride(0) < 2 ** 31):
        raise ValueError("%s: out must be float32 [%d, 3] on %s with adjacent columns (a column slice of wider rows is fine)"
                         % (what, M, dev))
    return out, int(out.stride(0)) if M > 1 else 3


def sample_image(pts_2d_or_pix, image, mode="rgb", normalize=True, channel_order="rgb", out=None, valid=None, row_begin=None,
                 row_count=None, max_rows=None, err=None):
    """``(colors float32 [M, 3], valid bool [M])``: the colour of the pixel under each point -- the loop of
    data_utils/ColorGenerator_Loader.py:63-65 and the divisions of :68-69, one ``pn2_sample_image`` launch.  ``pts_2d_or_pix``: int32
    ``[M, 2]`` pixels ``(x = column, y = row)`` as ``project_3d_to_2d(..., return_pixels=True)`` gives them, or float ``[M, 2]``
    (cast as ``to_pixels`` does).  ``image``: uint8 ``[H, W, 3]`` or ``[B, H, W, 3]`` on the device, its bytes in ``channel_order``
    (``"bgr"``: a ``cv2.imread`` frame, read in place).  ``mode="rgb"``: R, G, B; ``"hsv"``: OpenCV's 8-bit H (0 .. 179), S, V
    by the integer rule of include/pn2.h (UNVERIFIED against OpenCV, see the module docstring).  ``normalize``: divided by 255
    (the hue by 180) in float32, as the reference stores them.  A point outside the image (or unprojectable) gets three zeros and
    ``valid = False``; there is no depth test.

    ``out``: float32 ``[M, 3]`` to write into; a column slice of wider rows (``rows[:, 4:7]``) is painted in place.  ``valid``: a
    uint8 or bool ``[M]`` buffer.  ``row_begin`` / ``row_count`` (int64 ``[B]`` on the device) and ``max_rows`` (host bound of every
    count; default ``M``): cloud ``b`` is rows ``[row_begin[b], row_begin[b] + row_count[b])`` and reads ``image[b]``; rows beyond a
    count, or beyond ``max_rows``, are not touched (zeros where this call allocated them).  A cloud whose rows would leave
    ``[0, M)`` -- a stale count or begin -- is skipped whole, nothing of it read or written, and ``err`` (a zeroed device int32
    tensor of one element, optional) receives ``_lib.IMAGE_ERR_ROWS``.
    Nothing is read back: with ``out`` and ``valid`` given (and int32 pixels) the call allocates nothing and can be captured."""
    if not isinstance(pts_2d_or_pix, torch.Tensor) or not pts_2d_or_pix.is_cuda or not isinstance(image, torch.Tensor) or not image.is_cuda:
        raise _lib.Pn2Error("sample_image: points and image must live on the GPU: this package has no CPU path")
    if pts_2d_or_pix.dim() != 2 or pts_2d_or_pix.shape[1] != 2:
        raise AssertionError(tuple(pts_2d_or_pix.shape))
    dev = pts_2d_or_pix.device
    pix = pts_2d_or_pix.contiguous() if pts_2d_or_pix.dtype == torch.int32 else to_pixels(pts_2d_or_pix.detach())
    M = int(pix.shape[0])
    if image.dtype != torch.uint8 or image.dim() not in (3, 4) or image.shape[-1] != 3 or image.device != dev:
        raise ValueError("sample_image: image must be uint8 [H, W, 3] or [B, H, W, 3] on %s" % dev)
    image = image.contiguous()
    B = int(image.shape[0]) if image.dim() == 4 else 1
    H, W = int(image.shape[-3]), int(image.shape[-2])
    if H < 1 or W < 1 or H * W * 3 >= 2 ** 31:
        raise ValueError("sample_image: an image must hold 1 <= H * W * 3 < 2^31 bytes")
    if (row_begin is None) != (row_count is None) or (row_count is None and B != 1):
        raise ValueError("sample_image: row_begin and row_count come together, and a batch of images needs them")
    for t in (row_begin, row_count):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.device != dev or t.numel() != B
                              or not t.is_contiguous()):
            raise ValueError("sample_image: row_begin / row_count must be contiguous int64 [%d] tensors on %s" % (B, dev))
    max_rows = M if max_rows is None else int(max_rows)
    if not 0 <= max_rows <= M:
        raise ValueError("sample_image: max_rows must lie in [0, %d]" % M)
    partial = row_count is not None or max_rows < M                  # rows may stay untouched: what is allocated here is zeroed
    out, ldo = _color_rows(out, M, dev, "sample_image", partial)
    if err is not None and (not isinstance(err, torch.Tensor) or err.dtype != torch.int32 or err.numel() != 1 or err.device != dev):
        raise ValueError("sample_image: err must be an int32 tensor of one element on %s" % dev)
    order, what = _code(_ORDERS, channel_order, "channel_order"), _code(_MODES, mode, "mode")
    if valid is None:
        valid = (torch.zeros if partial else torch.empty)(M, device=dev, dtype=torch.uint8)
    elif not isinstance(valid, torch.Tensor) or valid.dtype not in (torch.uint8, torch.bool) or valid.shape != (M,) or \
            not valid.is_contiguous() or valid.device != dev:
        raise ValueError("sample_image: valid must be a contiguous uint8 or bool [%d] tensor on %s" % (M, dev))
    if max_rows > 0:
        _check(_lib.load().pn2_sample_image(_p(pix), _p(image), B, H, W, order, what, int(bool(normalize)), _p(row_begin),
                                            _p(row_count), max_rows, M, _p(out), ldo, _p(valid), _p(err), _lib.stream()),
               "pn2_sample_image")
    return out, valid.view(torch.bool)


def paint_points(points, calib, image, mode="rgb", normalize=True, channel_order="rgb", out=None, pix=None, valid=None,
                 row_begin=None, row_count=None, max_rows=None, return_valid=False, err=None):
    """``[M, C + 3]`` float32 rows: ``points`` (float32 ``[M, C >= 3]``, velodyne x, y, z first) with the camera colour of each point
    appended -- ``project_3d_to_2d`` then ``sample_image`` (two launches of the library, nothing read back), the first step of the
    colour-generation task (ColorGenerator_Loader.py:58-71: ``[M, 7]`` rows x, y, z, i, c0, c1, c2).  ``image`` and the colour
    arguments are ``sample_image``'s; for a batch (``image`` ``[B, H, W, 3]`` with ``row_begin`` / ``row_count``) one calibration
    serves all clouds.  ``out``: contiguous float32 ``[M, C + 3]`` to write into (``out[:, :C]`` may BE ``points``: nothing is
    copied then); ``pix``: int32 ``[M, 2]``, ``valid``: uint8 / bool ``[M]`` buffers.  With all three given the call allocates
    nothing and can be captured.  ``return_valid``: return ``(rows, valid bool [M])``.  Rows outside every count (or beyond
    ``max_rows``) keep their points and get NO colour: zeros where this call allocated ``out``, whatever a given ``out`` held.
    ``err``: ``sample_image``'s."""
    pts, M, _ = _xyz_rows(points, "paint_points")
    C, dev = int(points.shape[1]), pts.device
    if out is None:
        partial = row_count is not None or (max_rows is not None and int(max_rows) < M)
        out = (torch.zeros if partial else torch.empty)(M, C + 3, device=dev, dtype=torch.float32)
    elif not isinstance(out, torch.Tensor) or out.shape != (M, C + 3) or out.dtype != torch.float32 or not out.is_contiguous() or \
            out.device != dev:
        raise ValueError("paint_points: out must be a contiguous float32 [%d, %d] tensor on %s" % (M, C + 3, dev))
    if M > 0 and not (points.data_ptr() == out.data_ptr() and tuple(points.stride()) == (C + 3, 1)):
        out[:, :C].copy_(points.detach())
    if pix is None:
        pix = torch.empty(M, 2, device=dev, dtype=torch.int32)
    _project_pixels(out, M, C + 3, calib, pix)
    _, valid = sample_image(pix, image, mode, normalize, channel_order, out[:, C:], valid, row_begin, row_count, max_rows, err)
    return (out, valid) if return_valid else out


def _project_pixels(rows, M, ld, calib, pix):
    """The pixels alone (``pn2_project_points`` with a NULL ``pts_2d``) of the first three columns of contiguous rows."""
    if pix.shape != (M, 2) or pix.dtype != torch.int32 or not pix.is_contiguous() or pix.device != rows.device:
        raise ValueError("paint_points: pix must be a contiguous int32 [%d, 2] tensor on %s" % (M, rows.device))
    if M > 0:
        _check(_lib.load().pn2_project_points(_p(rows), ld, M, calib.RT.ctypes.data_as(ctypes.c_void_p),
                                              calib.P.ctypes.data_as(ctypes.c_void_p), None, _p(pix), _lib.stream()),
               "pn2_project_points")


def hsv_to_rgb(colors, channel_order="rgb", out=None):
    """uint8 ``[..., 3]`` pixels of normalised HSV rows float32 ``[..., 3]`` (h in units of 180, s and v in units of 255: what
    ``sample_image(mode="hsv")`` writes and ``PointNetColorGen`` predicts) -- for LOOKING at a prediction, the step the reference
    has commented out (ColorGenerator_Loader.py:66-67).  This package's own fp64 definition (include/pn2.h, ``pn2_hsv_to_rgb``:
    s and v clamped to [0, 1], the hue wrapped, round-half-even), not OpenCV's float-based ``HSV2RGB`` bit for bit.  A NaN gives a
    black pixel.  A column slice of wider rows is read in place.  ``out``: a contiguous uint8 tensor of as many elements."""
    if not isinstance(colors, torch.Tensor) or not colors.is_cuda:
        raise _lib.Pn2Error("hsv_to_rgb: colors must live on the GPU: this package has no CPU path")
    if colors.dtype != torch.float32:
        raise RuntimeError("hsv_to_rgb: colors must be float32 (got %s)" % colors.dtype)
    if colors.dim() < 1 or colors.shape[-1] != 3:
        raise AssertionError(tuple(colors.shape))
    shape = tuple(colors.shape)
    rows = colors.detach()
    if rows.dim() != 2 or (rows.shape[0] > 0 and rows.stride(1) != 1) or (rows.shape[0] > 1 and not 3 <= rows.stride(0) < 2 ** 31):
        rows = rows.reshape(-1, 3).contiguous()
    N = int(rows.shape[0])
    if out is None:
        out = torch.empty(shape, device=rows.device, dtype=torch.uint8)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.numel() != 3 * N or not out.is_contiguous() or \
            out.device != rows.device:
        raise ValueError("hsv_to_rgb: out must be a contiguous uint8 tensor of %d elements on %s" % (3 * N, rows.device))
    order = _code(_ORDERS, channel_order, "channel_order")
    if N > 0:
        _check(_lib.load().pn2_hsv_to_rgb(_p(rows), int(rows.stride(0)) if N > 1 else 3, N, order, _p(out), _lib.stream()),
               "pn2_hsv_to_rgb")
    return out


# ----------------------------------------------------------------------------------------------------------------- ego view
class PinholeCamera:
    """``extrinsic`` ``[4, 4]`` (world -> camera; +X right, +Y down, +Z forward, open3d's convention), ``intrinsic`` ``[3, 3]``
    (float64) and the image's ``width`` / ``height``.  ``E`` is the ``[3, 4]`` block ``[R | t]`` and ``K`` the four numbers
    ``fx, fy, cx, cy`` that ``pn2_depth_splat`` reads; a skewed intrinsic matrix is refused."""

    def __init__(self, extrinsic, intrinsic, width, height):
        self.extrinsic = np.ascontiguousarray(extrinsic, np.float64).reshape(4, 4)
        self.intrinsic = np.ascontiguousarray(intrinsic, np.float64).reshape(3, 3)
        self.width, self.height = int(width), int(height)
        if self.width <= 0 or self.height <= 0:
            raise ValueError("PinholeCamera: width and height must be positive")
        k = self.intrinsic
        if k[0, 1] != 0 or k[1, 0] != 0 or k[2, 0] != 0 or k[2, 1] != 0 or k[2, 2] != 1:
            raise ValueError("PinholeCamera: the intrinsic matrix must be [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]")
        self.E = np.ascontiguousarray(self.extrinsic[:3, :])
        self.K = np.array([k[0, 0], k[1, 1], k[0, 2], k[1, 2]], np.float64)

    @classmethod
    def from_json(cls, fn):
        """An open3d ``PinholeCameraParameters`` file (the reference's ``config/ego_view.json``): ``extrinsic`` holds 16 numbers and
        ``intrinsic.intrinsic_matrix`` 9, both COLUMN-major (so the translation is extrinsic numbers 12, 13 and 14);
        keys this class does not know (``h_fov``, ``d_range``, ...) are ignored."""
        with open(fn, "r") as f:
            d = json.load(f)
        intr = d["intrinsic"]
        ext = np.array(d["extrinsic"], np.float64)
        mat = np.array(intr["intrinsic_matrix"], np.float64)
        if ext.shape != (16,) or mat.shape != (9,):
            raise ValueError("%s: extrinsic must hold 16 numbers and intrinsic.intrinsic_matrix 9" % fn)
        return cls(ext.reshape(4, 4).T, mat.reshape(3, 3).T, intr["width"], intr["height"])


class RenderOption:
    """``point_size`` (int) and ``background_color`` (a uint8 triple) of an open3d ``RenderOption``; nothing else of it is used."""

    def __init__(self, point_size=2, background_color=(0, 0, 0)):
        if int(point_size) != point_size:
            raise ValueError("RenderOption: point_size %r is not an integer (only whole point sizes are drawn)" % (point_size,))
        self.point_size = int(point_size)
        self.background_color = tuple(int(c) for c in background_color)
        if len(self.background_color) != 3 or not all(0 <= c <= 255 for c in self.background_color):
            raise ValueError("RenderOption: background_color must be three values in 0 .. 255")

    @classmethod
    def from_json(cls, fn):
        """An open3d ``RenderOption`` file (the reference's ``config/render_option.json``): ``point_size`` as an int (a non-integer
        size raises ``ValueError``), ``background_color`` (floats in [0, 1]) as ``round(c * 255)``.  A missing key takes this
        class's default (2, black); every other key is ignored."""
        with open(fn, "r") as f:
            d = json.load(f)
        bg = d.get("background_color", (0.0, 0.0, 0.0))
        if len(bg) != 3 or not all(0.0 <= float(c) <= 1.0 for c in bg):
            raise ValueError("%s: background_color must be three floats in [0, 1]" % fn)
        return cls(d.get("point_size", 2), tuple(int(round(float(c) * 255)) for c in bg))


def _buffer(t, numel, itemsize, dev, what):
    if not isinstance(t, torch.Tensor) or t.numel() != numel or t.element_size() != itemsize or not t.is_contiguous() or t.device != dev:
        raise ValueError("render_points: %s must be a contiguous %d-byte tensor of %d elements on %s" % (what, itemsize, numel, dev))
    return t


def render_points(pts_3d, labels, colors, camera, point_size=2, background=(0, 0, 0), near=0.1, far=1000.0, out=None, zkey=None,
                  owner=None, depth=None, err=None, return_depth=False, return_index=False):
    """The 3-D ego view of ``Window_Manager.update`` (pcdvis.py:31-51): uint8 ``[H, W, 3]`` on the device, ``H, W`` the camera's.
    ``pts_3d``: float32 ``[N, >= 3]`` (the first three columns of scan rows are read in place), ``labels`` int64 ``[N]``, ``colors``
    uint8 ``[C, 3]``, as for ``draw_2d_points``.  Point ``i`` is a square of ``point_size`` pixels (1 .. 16) of ``colors[labels[i]]``
    around its projection through ``camera`` (a ``PinholeCamera``); every pixel shows the NEAREST point that covers it, the
    lowest index among points of equal float32 depth; a pixel no point covers shows ``background`` (a colour triple, or a uint8
    ``[H, W, 3]`` image, not modified).  Points with a camera depth outside ``(near, far)`` are not drawn.  The rule is written
    out in include/pn2.h (``pn2_depth_splat``) and is UNVERIFIED AGAINST OPEN3D, as are the defaults ``near = 0.1`` and
    ``far = 1000``: they are this package's choice, open3d derives its planes from the scene's bounding box (module docstring).

    ``return_depth`` adds float32 ``[H, W]``, the visible point's camera depth (``+inf``: empty); ``return_index`` adds int32
    ``[H, W]``, its index (``-1``: empty) -- the range / index image of the cloud; the return value is then a tuple in that order.

    A label outside ``[0, C)`` leaves the background and sets ``err`` (a zeroed device int32 tensor); without ``err`` the flag is
    read back and raises ``IndexError`` (skipped under stream capture).  ``out``, ``zkey`` (64-bit, ``[H * W]``), ``owner``
    (32-bit, ``[H * W]``) and ``depth`` (float32, ``[H * W]`` elements): buffers to write into.  With ``out``, ``zkey``, ``owner``
    and ``err`` given (and ``depth`` if it is asked for, and a black or an image background) the image is drawn without an
    allocation or a read-back, so the call can be captured in a graph."""
    if not isinstance(labels, torch.Tensor) or not labels.is_cuda:
        raise _lib.Pn2Error("render_points: points and labels must live on the GPU: this package has no CPU path")
    pts, N, ld = _xyz_rows(pts_3d, "render_points")
    dev = pts.device
    if int(point_size) != point_size:
        raise ValueError("render_points: point_size %r is not an integer" % (point_size,))
    if labels.numel() != N or labels.dtype != torch.int64:
        raise ValueError("render_points: labels must be int64 [%d]" % N)
    labels = labels.reshape(-1).contiguous()
    colors = _dev_u8(colors, dev, "colors")
    if colors.dim() != 2 or colors.shape[1] != 3:
        raise ValueError("render_points: colors must be [C, 3]")
    H, W = camera.height, camera.width
    if isinstance(background, (torch.Tensor, np.ndarray)):
        background = _dev_u8(background, dev, "background")
        if background.shape != (H, W, 3):
            raise ValueError("render_points: a background image must be [%d, %d, 3]" % (H, W))
    else:
        bg = tuple(int(c) for c in background)
        if len(bg) != 3 or not all(0 <= c <= 255 for c in bg):
            raise ValueError("render_points: a background colour must be three values in 0 .. 255")
        background = None if bg == (0, 0, 0) else torch.tensor(bg, device=dev, dtype=torch.uint8).expand(H, W, 3).contiguous()
    if out is None:
        out = torch.empty(H, W, 3, device=dev, dtype=torch.uint8)
    elif out.shape != (H, W, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != dev:
        raise ValueError("render_points: out must be a contiguous uint8 [%d, %d, 3] tensor on %s" % (H, W, dev))
    zkey = torch.empty(H * W, device=dev, dtype=torch.int64) if zkey is None else _buffer(zkey, H * W, 8, dev, "zkey")
    owner = torch.empty(H * W, device=dev, dtype=torch.int32) if owner is None else _buffer(owner, H * W, 4, dev, "owner")
    if depth is None and return_depth:
        depth = torch.empty(H, W, device=dev, dtype=torch.float32)
    if depth is not None:
        if depth.dtype != torch.float32:
            raise RuntimeError("render_points: depth must be float32 (got %s)" % depth.dtype)
        _buffer(depth, H * W, 4, dev, "depth")
    flag = err if err is not None else torch.zeros(1, device=dev, dtype=torch.int32)
    lib, st = _lib.load(), _lib.stream()
    _check(lib.pn2_depth_splat(_p(pts) if N > 0 else None, ld, N, camera.E.ctypes.data_as(ctypes.c_void_p),
                               camera.K.ctypes.data_as(ctypes.c_void_p), float(near), float(far), int(point_size), H, W, _p(zkey), st),
           "pn2_depth_splat")
    _check(lib.pn2_depth_resolve(_p(zkey), H, W, _p(owner), _p(depth), st), "pn2_depth_resolve")
    _check(lib.pn2_splat_resolve(_p(owner), H, W, _p(labels), N, _p(colors), int(colors.shape[0]), _p(background), _p(out), _p(flag), st),
           "pn2_splat_resolve")
    if err is None and not torch.cuda.is_current_stream_capturing() and int(flag.item()) != 0:
        raise IndexError("render_points: a label is outside [0, %d)" % colors.shape[0])
    ret = (out,)
    if return_depth:
        ret += (depth.view(H, W),)
    if return_index:
        ret += (owner.view(torch.int32).view(H, W) - 1,)
    return ret if len(ret) > 1 else out


# -------------------------------------------------------------------------------------------------------------------- frame
class InstanceSpec:
    """How ``FrameSegmenter.label_scan(instances=)`` makes instances: cells ``voxel_size`` METRES wide (a scalar), ``things`` -- the
    predicted classes that get instance ids (for SemanticKITTI's shifted training classes ``range(8)``: car .. motorcyclist) --,
    ``connectivity`` 6 / 18 / 26 and ``min_points``, the fewest rows of an instance (smaller components get no id).  ``boxes=True``: an
    oriented box per instance as well (``boxes.instance_boxes`` with a table of ``box_angles`` angles and the closeness floor ``box_d0``
    in metres)."""

    def __init__(self, voxel_size, things, connectivity=26, min_points=1, boxes=False, box_angles=64, box_d0=0.05):
        self.voxel_size, self.things = float(voxel_size), sorted(set(int(t) for t in things))
        self.connectivity, self.min_points = int(connectivity), int(min_points)
        if not self.things or self.things[0] < 0 or connectivity not in (6, 18, 26) or self.min_points < 1 or not self.voxel_size > 0:
            raise ValueError("InstanceSpec: voxel_size > 0, at least one class >= 0 in things, connectivity 6 / 18 / 26, min_points >= 1")
        self.boxes, self.box_angles, self.box_d0 = bool(boxes), int(box_angles), float(box_d0)
        if not 1 <= self.box_angles <= _lib.BOX_MAX_ANGLES or not math.isfinite(self.box_d0):
            raise ValueError("InstanceSpec: 1 <= box_angles <= %d, box_d0 finite" % _lib.BOX_MAX_ANGLES)
        self._member = {}

    def member(self, device):
        """The class set as ``VoxelGrid.components``' ``member``: int32 ``[max(things) + 1]`` on ``device`` (made once)."""
        key = str(device)
        if key not in self._member:
            flags = torch.zeros(self.things[-1] + 1, dtype=torch.int32)
            flags[self.things] = 1
            self._member[key] = flags.to(device)
        return self._member[key]


class FrameSegmenter:
    """The body of the reference's frame loop (pcdvis.py:116-144) for one scan ``[M, 4]`` (x, y, z, intensity, as
    ``kitti.read_scan`` returns it): resample to ``npoints`` rows, normalise (``pn2_prepare_clouds``), run ``model`` in eval
    mode, predict, project the resampled un-normalised xyz into the camera and draw both views.

    ``colors`` uint8 ``[C, 3]`` (one row per class, or per group with ``groups``); ``groups``: a ``merge_groups`` table, the
    prediction is then taken over the merged classes.  ``frame`` returns a dict of device tensors -- ``pred`` int64 ``[N]``,
    ``log_probs`` ``[N, C]``, ``points`` (normalised, ``[N, 4]``), ``pts_3d`` ``[N, 3]``, ``pts_2d`` float32 ``[N, 2]``, ``pix``,
    ``image`` uint8 ``[H, W, 3]`` and ``top_view`` uint8 ``[600, 800, 3]`` -- and reads nothing back.  The outputs are buffers owned
    by the segmenter and overwritten by the next frame.  ``error_flag`` (device int32, cleared at the start of every ``frame``;
    ``render`` alone only ever sets it) becomes non-zero if a predicted label had
    no colour or a ``choice`` lay outside the scan.  ``render(log_probs, raw_rows, points)`` is the post-network part alone: it allocates nothing, so it can be
    captured in a graph.

    ``frame_raw`` starts from the RAW scan (``kitti.ScanFilter`` on the device); ``label_scan`` is ``frame_raw`` plus a label for
    every row of the scan (the k nearest drawn rows vote: ``pointnet_util.propagate_labels``), for ``kitti.write_labels``.

    ``camera`` (a ``PinholeCamera``): ``render`` then also draws the 3-D ego view of the un-normalised points (pcdvis.py:143,
    ``render_points`` with ``point_size`` on ``ego_background``, a colour triple) into ``ego_view`` uint8
    ``[camera.height, camera.width, 3]``, and ``frame`` returns it under ``"ego_view"``.  Without a camera there is no such key, buffer or launch.

    ``frame`` / ``frame_raw`` / ``label_scan(..., image=)``: the camera frame (uint8 ``[H, W, 3]``, bytes in ``channel_order``).  The
    result then gains ``"point_colors"`` float32 ``[N, 3]`` and ``"point_valid"`` bool ``[N]``: the colour of the pixel under each DRAWN
    row (``sample_image`` on ``pix`` with ``color_mode`` / ``color_normalize``), e.g. the colour-generation task's target for this
    frame.  ``image=None`` leaves all three calls exactly as they are: no key, buffer or launch."""

    def __init__(self, model, calib, colors, npoints=25000, image_size=(375, 1242), groups=None, radius=2, device="cuda", camera=None,
                 point_size=2, ego_background=(0, 0, 0), color_mode="rgb", color_normalize=True, channel_order="rgb"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.Pn2Error("FrameSegmenter: the HIP device is the only implementation")
        self.model, self.calib, self.groups = model, calib, _as_groups(groups)
        self.npoints, self.radius = int(npoints), int(radius)
        self.image_size = (int(image_size[0]), int(image_size[1]))
        _half_widths(self.radius, None)
        self.colors = _dev_u8(colors, self.device, "colors")
        n, dev, (H, W) = self.npoints, self.device, self.image_size
        self.raw_rows = torch.empty(n, 4, device=dev, dtype=torch.float32)
        self.pred = torch.empty(n, device=dev, dtype=torch.int64)
        self.pts_2d = torch.empty(n, 2, device=dev, dtype=torch.float32)
        self.pix = torch.empty(n, 2, device=dev, dtype=torch.int32)
        self.top_pix = torch.empty(n, 2, device=dev, dtype=torch.int32)
        self.image = torch.empty(H, W, 3, device=dev, dtype=torch.uint8)
        self.top_view = torch.empty(600, 800, 3, device=dev, dtype=torch.uint8)
        self.camera, self.point_size = camera, RenderOption(point_size).point_size
        ego = 0 if camera is None else camera.height * camera.width
        self._owner = torch.empty(max(H * W, 600 * 800, ego), device=dev, dtype=torch.int32)
        if camera is not None:
            self.ego_view = torch.empty(camera.height, camera.width, 3, device=dev, dtype=torch.uint8)
            self._zkey = torch.empty(ego, device=dev, dtype=torch.int64)
            bg = RenderOption(self.point_size, ego_background).background_color
            self._ego_background = bg if bg == (0, 0, 0) else \
                torch.tensor(bg, device=dev, dtype=torch.uint8).expand(camera.height, camera.width, 3).contiguous()
        self.error_flag = torch.zeros(1, device=dev, dtype=torch.int32)
        _code(_MODES, color_mode, "color_mode")
        _code(_ORDERS, channel_order, "channel_order")
        self.color_mode, self.color_normalize, self.channel_order = color_mode, bool(color_normalize), channel_order
        self.point_colors = self._point_valid = None                 # made by the first frame that comes with an image

    def choice(self, length, rng="numpy"):
        """``np.random.choice(length, npoints, replace=True)`` (pcdvis.py:121: a seeded numpy run draws what the reference
        draws), or the same distribution from a device ``torch.Generator``.  With a generator ``length`` may be a device int64
        tensor of one element (``ScanFilter.filter``'s count): the draw is ``min((u * length).long(), length - 1)`` on the device,
        nothing is read back, and a length of 0 gives -1 everywhere.  ``rng="cover"`` draws nothing: ``choice[i] = i % length``,
        computed on the device (``length`` an int or such a tensor; 0 gives -1 everywhere) -- with ``length <= npoints`` every row
        is taken at least once, which is what a voxel-grid subsample (``frame_raw(voxel=...)``) wants."""
        if isinstance(rng, str) and rng == "cover":
            i = torch.arange(self.npoints, device=self.device, dtype=torch.int64)
            if isinstance(length, torch.Tensor):
                return torch.where(length > 0, torch.remainder(i, length.clamp(min=1)), -1)
            return torch.remainder(i, length) if length > 0 else torch.full_like(i, -1)
        if isinstance(rng, torch.Generator):
            u = torch.rand(self.npoints, device=self.device, dtype=torch.float64, generator=rng)
            if isinstance(length, torch.Tensor):
                return torch.minimum((u * length).long(), length - 1)
            return torch.clamp((u * length).long(), max=length - 1)
        if rng != "numpy":
            raise ValueError('FrameSegmenter: rng must be "numpy", "cover" or a device torch.Generator')
        return torch.from_numpy(np.random.choice(int(length), self.npoints, replace=True).astype(np.int64)).to(self.device)

    def render(self, log_probs, raw_rows, points, background=None):
        """Post-network stages into the segmenter's buffers: predict, project ``raw_rows[:, :3]``, draw the camera image over
        ``background`` and the top view of the normalised ``points``; with a camera, the ego view of ``raw_rows[:, :3]`` too."""
        H, W = self.image_size
        predict(log_probs, self.groups, out=self.pred)
        project_3d_to_2d(raw_rows, self.calib, out=(self.pts_2d, self.pix))
        draw_2d_points(self.pix, self.pred, self.colors, background, self.image_size, self.radius, None, self.image,
                       self._owner[:H * W], self.error_flag)
        top_view_pixels(points, out=self.top_pix)
        draw_2d_points(self.top_pix, self.pred, self.colors, None, (600, 800), 3, None, self.top_view, self._owner[:600 * 800],
                       self.error_flag)
        if self.camera is not None:
            render_points(raw_rows, self.pred, self.colors, self.camera, self.point_size, self._ego_background, out=self.ego_view,
                          zkey=self._zkey, owner=self._owner[:self.camera.height * self.camera.width], err=self.error_flag)

    def frame(self, points, background=None, choice=None, rng="numpy", image=None):
        lib = _lib.load()
        self.error_flag.zero_()                                      # per frame; an async fill, nothing is read back
        if isinstance(points, np.ndarray):
            points = torch.from_numpy(np.ascontiguousarray(points, np.float32))
        if points.dim() != 2 or points.shape[1] != 4 or points.dtype != torch.float32:
            raise ValueError("FrameSegmenter.frame: points must be float32 [M, 4] (x, y, z, intensity)")
        raw = points.to(self.device).contiguous()
        M = int(raw.shape[0])
        if M == 0:
            raise ValueError("FrameSegmenter.frame: empty scan")
        if choice is None:
            choice = self.choice(M, rng)
        choice = torch.as_tensor(choice).to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
        if choice.numel() != self.npoints:
            raise ValueError("FrameSegmenter.frame: choice must hold npoints = %d rows" % self.npoints)
        n = self.npoints
        begin = torch.zeros(1, device=self.device, dtype=torch.int64)
        count = torch.full((1,), M, device=self.device, dtype=torch.int64)
        normed = torch.empty(1, n, 4, device=self.device, dtype=torch.float32)
        # (a choice outside the scan sets error_flag and reads row 0 / zeros: numpy raises IndexError)
        _check(lib.pn2_prepare_clouds(_p(raw), _p(begin), _p(count), None, None, None, _p(choice), 1, n, _p(normed), None,
                                      _p(self.error_flag), _lib.stream()), "pn2_prepare_clouds")
        # the resampled raw rows (pcdvis.py:122, :125) through the library's row gather: [1, M, 4] -> [1, n, 4]
        _check(lib.pn2_gather_rows(_p(raw), _p(choice), 1, M, 4, n, _p(self.raw_rows), _p(self.error_flag), _lib.stream()),
               "pn2_gather_rows")
        return self._finish(normed, background, image)

    def _finish(self, normed, background, image=None):
        """The network and the post-network stages on the normalised rows ``[1, n, 4]`` (``self.raw_rows`` holds the raw ones)."""
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                log_probs = self.model(normed.transpose(2, 1))
        finally:
            self.model.train(was_training)
        if isinstance(log_probs, (tuple, list)):                     # 'pointnet' returns (pred, trans_feat)
            log_probs = log_probs[0]
        log_probs = log_probs[0]
        if background is not None:
            background = _dev_u8(background, self.device, "background")
        self.render(log_probs, self.raw_rows, normed[0], background)
        out = {"pred": self.pred, "log_probs": log_probs, "points": normed[0], "pts_3d": self.raw_rows[:, :3],
               "pts_2d": self.pts_2d, "pix": self.pix, "image": self.image, "top_view": self.top_view}
        if self.camera is not None:
            out["ego_view"] = self.ego_view
        if image is not None:
            # the camera colour under every drawn row (sample_image on the pixels just projected): buffers made on first use
            if self.point_colors is None:
                self.point_colors = torch.empty(self.npoints, 3, device=self.device, dtype=torch.float32)
                self._point_valid = torch.empty(self.npoints, device=self.device, dtype=torch.uint8)
            image = _dev_u8(image, self.device, "image")
            _, valid = sample_image(self.pix, image, self.color_mode, self.color_normalize, self.channel_order, self.point_colors,
                                    self._point_valid)
            out["point_colors"], out["point_valid"] = self.point_colors, valid
        return out

    def _raw_buffers(self, scan_filter, rows):
        """Static input and ``ScanBuffers`` of capacity ``rows`` for ``frame_raw`` (kept while the capacity and the filter's device
        stay the same)."""
        held = getattr(self, "_raw_state", None)
        if held is None or held["rows"] < rows:
            dev = self.device
            held = {"rows": rows, "raw": torch.empty(rows, 4, device=dev, dtype=torch.float32),
                    "words": torch.empty(rows, device=dev, dtype=torch.int32), "out": scan_filter.buffers(rows),
                    "begin": torch.zeros(1, device=dev, dtype=torch.int64), "count": torch.zeros(1, device=dev, dtype=torch.int64)}
            self._raw_state = held
        return held

    def frame_raw(self, raw_scan, raw_label=None, scan_filter=None, rng="numpy", background=None, choice=None, max_rows=None,
                  voxel=None, image=None):
        """``frame`` for a RAW scan: ``raw_scan`` float32 ``[M, 4]`` (the ``.bin`` rows) and, if there is one, ``raw_label`` ``[M]``
        (the ``.label`` words, uint32 / int32; None: a live feed), as numpy arrays or tensors on either side.  ``scan_filter``: a
        ``kitti.ScanFilter`` (its class map, subset and ranges).  The stages are: upload into a static buffer of ``max_rows`` rows
        (default: the largest scan seen so far) -> ``pn2_scan_filter`` -> the choice -> ``pn2_prepare_clouds`` and the row
        gather with the DEVICE-side kept count -> the rest of ``frame``.  The result holds ``frame``'s keys plus ``count`` (int64
        ``[1]`` on the device), ``labels`` (int32, the kept rows' classes, None without ``raw_label``) and ``index`` (int32, their
        raw rows); only the first ``count`` entries of the last two mean anything.

        ``rng``: with a device ``torch.Generator`` the choice is ``min((u * count).long(), count - 1)`` on the device and NOTHING
        is read back (with ``raw_scan`` / ``raw_label`` already on the device, or pinned, the whole call is free of host
        synchronisation).  With ``rng="numpy"`` the ONE kept count is read back and ``np.random.choice(count, npoints)`` is
        drawn, which is the reference's draw (pcdvis.py:121) from a seeded numpy run.  An explicit ``choice`` (row numbers in the
        FILTERED scan) is used as it is.

        A scan of which nothing survives the filter makes the device choice -1 everywhere: ``pn2_prepare_clouds`` flags that in
        ``error_flag`` (the frame then shows row 0 / zeros); with ``rng="numpy"`` it raises ``ValueError``, as ``frame`` does for
        an empty scan.  A raw class outside the map or more rows than ``max_rows`` set ``scan_filter.error_flag``.

        ``voxel`` (a ``voxel.VoxelGrid``): the kept rows are downsampled to one row per occupied cell after the filter
        (``pn2_voxel_grid``), and the choice, ``pn2_prepare_clouds`` and the row gather then read the DOWNSAMPLED rows: the choice is
        drawn from the voxel count (on the device for a device generator and for ``rng="cover"``; ``rng="numpy"`` reads that one
        count back), and an explicit ``choice`` names downsampled rows.  The result gains ``voxel_count`` (int64 ``[1]`` on the
        device), ``voxel_index`` (int32: the RAW row of each voxel's representative, the grid's ``index`` composed with the
        filter's; the first ``voxel_count`` entries mean something) and ``voxel_inverse`` (int32: for each KEPT row the rank of its
        voxel, -1 for a row the grid dropped); ``count`` / ``labels`` / ``index`` stay the filter's.  The grid carries its own
        choice of representative: with ``VoxelGrid(reduce="mean")`` the rows the network sees (and ``raw_rows``, ``pts_3d``, the
        pixels) are the voxels' MEAN rows, no rows of the scan; ``voxel_index`` still names each voxel's lowest raw row, and nothing
        here reads a downsampled row back through it."""
        lib = _lib.load()
        if scan_filter is None:
            raise ValueError("FrameSegmenter.frame_raw: a kitti.ScanFilter is needed")
        self.error_flag.zero_()
        if isinstance(raw_scan, np.ndarray):
            raw_scan = torch.from_numpy(np.ascontiguousarray(raw_scan, np.float32))
        if raw_scan.dim() != 2 or raw_scan.shape[1] != 4 or raw_scan.dtype != torch.float32:
            raise ValueError("FrameSegmenter.frame_raw: raw_scan must be float32 [M, 4] (x, y, z, intensity)")
        M = int(raw_scan.shape[0])
        if M == 0:
            raise ValueError("FrameSegmenter.frame_raw: empty scan")
        if raw_label is not None:
            if isinstance(raw_label, np.ndarray):
                raw_label = torch.from_numpy(np.ascontiguousarray(raw_label).view(np.int32))
            if raw_label.numel() != M or raw_label.element_size() != 4 or raw_label.is_floating_point():
                raise ValueError("Scan and Label don't contain same number of points")
        held = self._raw_buffers(scan_filter, max(M, int(max_rows or 0)))
        # (asynchronous only from the device or from pinned memory; a pageable host array is copied before the call returns)
        held["raw"][:M].copy_(raw_scan, non_blocking=raw_scan.is_cuda or raw_scan.is_pinned())
        if raw_label is not None:
            held["words"][:M].copy_(raw_label.reshape(-1).view(torch.int32), non_blocking=raw_label.is_cuda or raw_label.is_pinned())
        held["count"].fill_(M)
        pts, labels, index, count = scan_filter.filter(held["raw"], held["words"] if raw_label is not None else None, held["begin"],
                                                       held["count"], held["rows"], out=held["out"])
        src, src_count = pts, count
        if voxel is not None:
            vb = held.get("voxel")
            if vb is None or (voxel.reduces and vb.reduce_workspace is None):       # (a reducing grid brings a workspace of its own)
                vb = held["voxel"] = voxel.buffers(held["rows"])
            src, _, v_index, src_count, v_inverse, _ = voxel.downsample(pts, None, held["begin"], count, held["rows"], out=vb)
        if choice is None:
            if isinstance(rng, torch.Generator) or (isinstance(rng, str) and rng == "cover"):
                choice = self.choice(src_count, rng)
            else:
                kept = int(src_count.item())                         # the one read-back of the numpy draw
                if kept == 0:
                    raise ValueError("FrameSegmenter.frame_raw: nothing of the scan survives the filter")
                choice = self.choice(kept, rng)
        choice = torch.as_tensor(choice).to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
        if choice.numel() != self.npoints:
            raise ValueError("FrameSegmenter.frame_raw: choice must hold npoints = %d rows" % self.npoints)
        n = self.npoints
        normed = torch.empty(1, n, 4, device=self.device, dtype=torch.float32)
        # (a choice outside [0, count) sets error_flag and reads row 0: the count is the kernel's own, in device memory)
        _check(lib.pn2_prepare_clouds(_p(src), _p(held["begin"]), _p(src_count), None, None, None, _p(choice), 1, n, _p(normed), None,
                                      _p(self.error_flag), _lib.stream()), "pn2_prepare_clouds")
        _check(lib.pn2_gather_rows(_p(src), _p(choice), 1, held["rows"], 4, n, _p(self.raw_rows), _p(self.error_flag), _lib.stream()),
               "pn2_gather_rows")
        out = self._finish(normed, background, image)
        out.update({"count": count, "labels": labels, "index": index})
        if voxel is not None:
            # (entries beyond the voxel count are whatever the buffer held: clamped, so that the gather stays inside `index`)
            raw_row = torch.gather(index, 0, v_index.long().clamp_(0, held["rows"] - 1))
            out.update({"voxel_count": src_count, "voxel_index": raw_row, "voxel_inverse": v_inverse})
        return out

    def label_scan(self, raw_scan, raw_label=None, scan_filter=None, rng="numpy", k=5, max_dist=1.0, lut=None, background=None,
                   choice=None, max_rows=None, voxel=None, instances=None, image=None, search="brute"):
        """``frame_raw``, then a label for EVERY row of the raw scan.  The network labels ``npoints`` rows drawn with
        replacement (about ``exp(-npoints / count)`` of the kept rows are never drawn); here each kept row takes the majority
        label of its ``k`` nearest drawn rows (``pointnet_util.propagate_labels``: queries = the kept rows' xyz with the
        device-side count, candidates = ``raw_rows[:, :3]`` carrying ``pred``, un-normalised, so ``max_dist`` is in METRES;
        ``max_dist=None``: no cut-off) and is written at its raw row (the filter's ``index``).  The result, ``"scan_labels"`` in
        the returned dict, is int32 ``[M]``: ``lut[class]`` (``lut``: ``kitti.inverse_label_lut``, the dataset's raw ids; None: the
        predicted class itself) for the kept rows, 0 -- "unlabeled" in SemanticKITTI -- for the rows the filter dropped and
        for a kept row with no drawn row within ``max_dist``.  ``kitti.write_labels`` writes it as a ``.label`` file.

        A row drawn several times is a candidate several times and votes once per copy: deliberate, the copies are the
        draw's weights.  With a device generator nothing is read back.  A predicted class outside ``lut`` gives 0 and sets
        ``error_flag``.  ``voxel``: as in ``frame_raw`` -- the network sees the downsampled rows, the queries remain ALL kept
        rows, so the result means what it meant.

        ``instances`` (an ``InstanceSpec``): an INSTANCE id for every row as well -- Euclidean clustering per predicted "thing"
        class, the usual panoptic post-process.  Each kept row's predicted class (the same vote, BEFORE ``lut``; -1 without a voter)
        is gridded in metres at ``instances.voxel_size`` with the majority class per cell (``VoxelGrid(label_reduce="mode")``), the
        cells are clustered with ``same_label=True``, ``member=instances.things`` and ``row_labels=`` those classes
        (``VoxelGrid.components``), and the result gains ``"scan_instances"`` int32 ``[M]``, written at the raw rows like
        ``scan_labels``: ``id + 1``, 0 for the rows the filter dropped and for rows without an instance (a class outside ``things``, a
        row that disagrees with its cell's majority, a component below ``min_points``); ``"instance_count"`` (int64 ``[1]`` on the
        device); ``"kept_classes"`` (int32: the kept rows' predicted classes, the first ``count`` entries mean something) and
        ``"kept_instances"`` (int32: their ids, -1 for none -- an ``inverse``-style map for ``voxel.segment_mean``).  With
        ``instances.boxes`` also ``"instance_boxes"``: a ``boxes.Boxes`` over the kept rows in metres, instance ``id`` at row ``id``
        (the first ``instance_count`` rows mean something; its error bits go to the instance grid's ``error_flag``).  Ids are numbered by
        each instance's lowest kept row.  With a device generator nothing is read back.  ``kitti.write_labels(fn, scan_labels,
        scan_instances)`` writes both halves of the ``.label`` words.  ``instances=None`` leaves this call exactly as it was.

        ``search``: ``propagate_labels``' -- ``"grid"`` searches on a uniform grid of ``max_dist`` cells instead of by brute force
        (it needs a ``max_dist``)."""
        from . import neighbors, pointnet_util as U
        out = self.frame_raw(raw_scan, raw_label, scan_filter, rng, background, choice, max_rows, voxel, image)
        held = self._raw_state
        rows, n, M = held["rows"], self.npoints, int(raw_scan.shape[0])
        k = int(k)
        work = held.get("knn")
        if work is None or work[0] != (rows, k):
            dev = self.device
            work = held["knn"] = ((rows, k), torch.empty(rows, k, device=dev, dtype=torch.int64),
                                  torch.empty(rows, k, device=dev, dtype=torch.float32), torch.empty(rows, device=dev, dtype=torch.int32))
        _, idx, dist, scan_labels = work
        grid_ws = ()
        if search == "grid":
            if held.get("grid_ws") is None or held["grid_ws"].numel() < neighbors.workspace_bytes(n, 1):
                held["grid_ws"] = torch.empty(neighbors.workspace_bytes(n, 1), device=self.device, dtype=torch.uint8)
            grid_ws = (held["grid_ws"],)
        scan_labels.zero_()
        U.propagate_labels(held["out"].points[:, :3].contiguous().view(1, rows, 3), self.raw_rows[:, :3].contiguous().view(1, n, 3),
                           self.pred.view(1, n), k=k, max_dist=max_dist, fill=0, lut=lut, dst=out["index"], out=scan_labels,
                           n_query=out["count"], err=self.error_flag, work=(idx, dist) + grid_ws, search=search)
        out["scan_labels"] = scan_labels[:M]
        if instances is not None:
            self._scan_instances(out, instances, held, idx, dist, k, max_dist, M)
        return out

    def _scan_instances(self, out, spec, held, idx, dist, k, max_dist, M):
        """``label_scan(instances=)``: the kept rows' classes from the neighbours ``propagate_labels`` left in ``idx`` / ``dist``, the
        grid, the components, the scatter to the raw rows.  Buffers are kept with the raw state; nothing is read back."""
        from . import voxel as VX
        lib, dev = _lib.load(), self.device
        rows, n = held["rows"], self.npoints
        work = held.get("instances")
        if work is None or work["key"] != (rows, spec.voxel_size):
            grid = VX.VoxelGrid(spec.voxel_size, device=dev, label_reduce="mode")
            work = held["instances"] = {"key": (rows, spec.voxel_size), "grid": grid, "down": grid.buffers(rows),
                                        "comp": grid.component_buffers(rows), "classes": torch.empty(rows, device=dev, dtype=torch.int32),
                                        "scan": torch.empty(rows + 1, device=dev, dtype=torch.int32),
                                        "row": torch.arange(rows, device=dev, dtype=torch.int64)}
        classes, grid = work["classes"], work["grid"]
        classes.fill_(-1)
        max_d2 = float("inf") if max_dist is None else float(np.float32(float(max_dist) ** 2))
        # the vote of propagate_labels again, without the lut and the scatter: class per KEPT row (the neighbours are still in idx / dist)
        _check(lib.pn2_knn_vote(_p(idx), _p(dist), _p(self.pred.view(1, n)), 1, rows, n, k, max_d2, _p(out["count"]), -1, None, 0, None, rows,
                                _p(classes), _p(self.error_flag), _lib.stream()), "pn2_knn_vote")
        pts = held["out"].points
        down = grid.downsample(pts, classes, held["begin"], out["count"], rows, out=work["down"])
        comps = grid.components(pts, down, row_labels=classes, connectivity=spec.connectivity, same_label=True, member=spec.member(dev),
                                min_points=spec.min_points, row_begin=held["begin"], row_count=out["count"], max_rows=rows, out=work["comp"])
        # id + 1 at the raw rows; the kept rows beyond the count go to a spare last entry
        live = work["row"] < out["count"]
        scan = work["scan"]
        scan.zero_()
        scan.scatter_(0, torch.where(live, out["index"].long().clamp_(0, rows - 1), rows), torch.where(live, comps.row_component + 1, 0))
        out.update({"scan_instances": scan[:M], "instance_count": comps.count, "kept_classes": classes,
                    "kept_instances": comps.row_component})
        if spec.boxes:
            from . import boxes as BX
            buf = work.get("boxes")
            if buf is None or buf.angles != spec.box_angles:
                buf = work["boxes"] = BX.buffers(rows, 1, rows, spec.box_angles, dev)
            # (the error bits join the grid's word, which downsample cleared: one word for the chain)
            out["instance_boxes"] = BX.segment_boxes(pts, comps.row_component, comps.count, angles=spec.box_angles, d0=spec.box_d0,
                                                     row_begin=held["begin"], row_count=out["count"], max_rows=rows, buffers=buf,
                                                     error_flag=grid.error_flag)
