"""Launcher of csrc/vis_errors.hip: the 3D error report of `visualize_from_instances` (reference cubercnn/vis/vis.py:95-171)
for all predictions of a dataset in one call -- the 2D-IoU match of every prediction to the ground truth of its image and category
and the seven errors of the matched pairs, summed in a fixed order.
"""
import torch

from .. import lib as _lib

ERR_NAMES = ("xy", "z", "w", "h", "l", "dim", "ry")


def _check(t, dtype, shape, name):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise ValueError(f"{name} must be a {dtype} tensor")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def _check_offsets(off, images, rows, name):
    _check(off, torch.int32, (images + 1,), name)
    o = off.cpu()
    if int(o[0]) != 0 or int(o[-1]) != rows or bool((o[1:] < o[:-1]).any()):
        raise ValueError(f"{name} must start at 0, never decrease and end at {rows}")


def match_errors(dt_box, dt_cat, dt_c2d, dt_z, dt_dims, dt_pose, dt_off, gt_box, gt_cat, gt_center, gt_dims, gt_pose, gt_off, K):
    """Rows ragged by image through dt_off / gt_off ((I+1,) int32 prefix offsets).  Detections: dt_box (D,4) XYWH, dt_cat (D,) int32,
    dt_c2d (D,2), dt_z (D,), dt_dims (D,3), dt_pose (D,9) or (D,3,3); ground truth: gt_box (G,4) XYWH, gt_cat (G,) int32, gt_center
    (G,3), gt_dims (G,3), gt_pose (G,9) or (G,3,3); K (I,9) or (I,3,3).  All float32 unless noted, contiguous, on one device.
    -> match (D,) int32 (global ground-truth row of the same image and category with the largest 2D IoU, the lowest row among equal
    ones, -1 below IoU 0.5), err (D,7) float32 [xy, z, w, h, l, dim, ry] (NaN where unmatched), sums (7,) float64 over the matched
    pairs, counts (2,) int64 (matched pairs, pairs with a valid ry).  Two calls give the same bits.
    ry is pytorch3d's `so3_relative_angle(R_dt, R_gt, cos_bound=1)` as READ FROM ITS SOURCE (pytorch3d is not installed, so this is
    not a measured parity): pi / 2 - (trace(R_dt R_gt^T) - 1) / 2, and NaN / not counted where the trace lies outside
    [-1 - 1e-4, 3 + 1e-4], where pytorch3d raises and the reference skips the pair for ry only."""
    f32, i32 = torch.float32, torch.int32
    if not isinstance(dt_off, torch.Tensor) or dt_off.dim() != 1 or dt_off.numel() < 1:
        raise ValueError("dt_off must be a (I + 1,) int32 tensor")
    I = dt_off.numel() - 1
    D = dt_box.shape[0] if isinstance(dt_box, torch.Tensor) and dt_box.dim() else -1
    G = gt_box.shape[0] if isinstance(gt_box, torch.Tensor) and gt_box.dim() else -1
    for t, shape, name in ((dt_box, (D, 4), "dt_box"), (dt_c2d, (D, 2), "dt_c2d"), (dt_z, (D,), "dt_z"), (dt_dims, (D, 3), "dt_dims"),
                           (gt_box, (G, 4), "gt_box"), (gt_center, (G, 3), "gt_center"), (gt_dims, (G, 3), "gt_dims")):
        _check(t, f32, shape, name)
    _check(dt_cat, i32, (D,), "dt_cat")
    _check(gt_cat, i32, (G,), "gt_cat")
    for t, n, name in ((dt_pose, D, "dt_pose"), (gt_pose, G, "gt_pose"), (K, I, "K")):
        _check(t, f32, (n, 3, 3) if isinstance(t, torch.Tensor) and t.dim() == 3 else (n, 9), name)
    _check_offsets(dt_off, I, D, "dt_off")
    _check_offsets(gt_off, I, G, "gt_off")
    tensors = (dt_box, dt_cat, dt_c2d, dt_z, dt_dims, dt_pose, dt_off, gt_box, gt_cat, gt_center, gt_dims, gt_pose, gt_off, K)
    if len({t.device for t in tensors}) != 1:
        raise ValueError("all inputs must live on one device")
    L = _lib.check_device(*tensors)
    dev = dt_box.device
    match = torch.empty(D, dtype=i32, device=dev)
    err = torch.empty((D, 7), dtype=f32, device=dev)
    sums = torch.empty(7, dtype=torch.float64, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    workspace = torch.empty(max(I, 1) * 9, dtype=torch.float64, device=dev)
    L.call("omni_match_errors", *[_lib.ptr(t) for t in tensors], I, D, G, _lib.ptr(match), _lib.ptr(err), _lib.ptr(sums), _lib.ptr(counts),
           _lib.ptr(workspace), _lib.stream_of(dt_box))
    return match, err, sums, counts
