"""Launchers of csrc/annotate.hip: the derived box fields of Omni3D annotations (`bbox3D_cam`, `bbox2D_proj`, `bbox2D_trunc`,
`truncation`, `behind_camera` and the counters behind `visibility`) for all boxes of all images of a dataset, one launch each --
`get_cuboid_verts` / `convert_3d_box_to_2d` / `estimate_truncation` / `estimate_visibility` of the reference
(cubercnn/util/math_util.py:221-259, 498-577, 745-758, 728-743), which handle one box or one image per call.  The arguments are
checked by `kernels/_args.py`.
"""
import numpy as np
import torch

from .. import lib as _lib
from . import _args

TILE = 16          # csrc/cuboid_cast.h


def _inputs(box3d, R, box_off, K, size):
    I = _args.offset_count(box_off, "box_off")
    N = _args.tensor(box3d, "box3d", torch.float32, (None, 6))[0]
    _args.matrices(R, N, "R")
    _args.matrices(K, I, "K")
    _args.tensor(size, "size", torch.int32, (I, 2))
    _args.offsets(box_off, "box_off", N)
    tensors = (box3d, R, box_off, K, size)
    _args.one_device(tensors)
    return I, N, tensors


def box_annotate(box3d, R, box_off, K, size, min_z=0.20):
    """box3d (N,6) [X,Y,Z,W,H,L], R (N,9) or (N,3,3), box_off (I+1,) int32 prefix offsets of the boxes of every image, K (I,9) or
    (I,3,3), size (I,2) int32 [W, H]; float32 unless noted, contiguous, on one device.
    -> verts3d (N,8,3), verts2d (N,8,3) [u, v, z], proj (N,4) XYXY, trunc (N,4) XYXY, truncation (N,) float64, behind (N,) uint8,
    fully_behind (N,) uint8, as include/omni3d_hip.h defines them under omni_box_annotate.  Two calls give the same bits.
    ValueError on a wrong dtype / shape / stride / offset / device before anything is launched; I == 0 or N == 0 launches nothing."""
    I, N, tensors = _inputs(box3d, R, box_off, K, size)
    L = _lib.check_device(*tensors)
    dev, f32 = box3d.device, torch.float32
    verts3d = torch.empty((N, 8, 3), dtype=f32, device=dev)
    verts2d = torch.empty((N, 8, 3), dtype=f32, device=dev)
    proj = torch.empty((N, 4), dtype=f32, device=dev)
    trunc = torch.empty((N, 4), dtype=f32, device=dev)
    truncation = torch.empty(N, dtype=torch.float64, device=dev)
    behind = torch.empty(N, dtype=torch.uint8, device=dev)
    fully = torch.empty(N, dtype=torch.uint8, device=dev)
    if I > 0 and N > 0:
        L.call("omni_box_annotate", *[_lib.ptr(t) for t in tensors], I, N, float(min_z), _lib.ptr(verts3d), _lib.ptr(verts2d),
               _lib.ptr(proj), _lib.ptr(trunc), _lib.ptr(truncation), _lib.ptr(behind), _lib.ptr(fully), _lib.stream_of(box3d))
    return verts3d, verts2d, proj, trunc, truncation, behind, fully


def visibility_ragged(box3d, R, box_off, K, size, zplane=0.05):
    """Inputs as `box_annotate`.  -> area (N,) int32: pixels of its image whose centre ray meets the box at depth >= zplane; visible
    (N,) int32: those where it is the nearest of the boxes OF ITS IMAGE (equal depths go to the lower row) -- the counters of
    `render.cuboid_depth` called once per image, from one launch.  visibility = visible / area.  Two calls give the same bits."""
    I, N, tensors = _inputs(box3d, R, box_off, K, size)
    if not zplane > 0:
        raise ValueError("zplane must be positive")
    wh = size.cpu().numpy().astype(np.int64)
    if I > 0 and int(wh.min()) <= 0:
        raise ValueError("size must hold positive [W, H]")
    tiles = ((wh[:, 0] + TILE - 1) // TILE) * ((wh[:, 1] + TILE - 1) // TILE) if I > 0 else np.zeros(0, np.int64)
    tile_off = np.concatenate(([0], np.cumsum(tiles)))
    if int(tile_off[-1]) >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 tiles of 16 x 16 pixels: split the dataset")
    L = _lib.check_device(*tensors)
    dev = box3d.device
    area = torch.zeros(N, dtype=torch.int32, device=dev)
    visible = torch.zeros(N, dtype=torch.int32, device=dev)
    if I > 0 and N > 0:
        tile_off_d = torch.from_numpy(tile_off.astype(np.int32)).to(dev)
        L.call("omni_visibility_ragged", *[_lib.ptr(t) for t in tensors], _lib.ptr(tile_off_d), I, N, int(tile_off[-1]), float(zplane),
               _lib.ptr(area), _lib.ptr(visible), _lib.stream_of(box3d))
    return area, visible
