"""Launcher of csrc/vis_errors.hip: the 3D error report of `visualize_from_instances` (reference cubercnn/vis/vis.py:95-171)
for all predictions of a dataset in one call -- the 2D-IoU match of every prediction to the ground truth of its image and category
and the seven errors of the matched pairs, summed in a fixed order.  The arguments are checked by `kernels/_args.py`.
"""
import torch

from .. import lib as _lib
from . import _args

ERR_NAMES = ("xy", "z", "w", "h", "l", "dim", "ry")


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
    I = _args.offset_count(dt_off, "dt_off")
    D = _args.tensor(dt_box, "dt_box", f32, (None, 4))[0]
    G = _args.tensor(gt_box, "gt_box", f32, (None, 4))[0]
    for t, name, shape in ((dt_c2d, "dt_c2d", (D, 2)), (dt_z, "dt_z", (D,)), (dt_dims, "dt_dims", (D, 3)), (gt_center, "gt_center", (G, 3)),
                           (gt_dims, "gt_dims", (G, 3))):
        _args.tensor(t, name, f32, shape)
    _args.tensor(dt_cat, "dt_cat", i32, (D,))
    _args.tensor(gt_cat, "gt_cat", i32, (G,))
    for t, n, name in ((dt_pose, D, "dt_pose"), (gt_pose, G, "gt_pose"), (K, I, "K")):
        _args.matrices(t, n, name)
    _args.offsets(dt_off, "dt_off", D)
    _args.offsets(gt_off, "gt_off", G, count=I)
    tensors = (dt_box, dt_cat, dt_c2d, dt_z, dt_dims, dt_pose, dt_off, gt_box, gt_cat, gt_center, gt_dims, gt_pose, gt_off, K)
    _args.one_device(tensors)
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
