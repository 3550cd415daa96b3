"""Launchers of csrc/augment.hip and csrc/warp.hip: Pillow's bilinear coefficient rows built on the device, the PIL-exact resize of a window
of an image (INPUT.CROP), the integer colour jitter (INPUT.COLOR_JITTER) and the projective warp (INPUT.CAMERA_ROTATION).  Nothing here
uploads a table, copies the source or reads back."""
import math

import numpy as np
import torch

from .. import lib as _lib
from . import _args

CROP_GRID_THREADS = 8192 * 256      # csrc/augment.hip grid_for: the resampling passes stride over more work items than this
JITTER_GRID_THREADS = 2048 * 256    # csrc/augment.hip JITTER_MAX_BLOCKS: the same for the jitter's two passes
WARP_GRID_THREADS = 2048 * 256      # csrc/warp.hip WARP_MAX_BLOCKS: the warp strides over more output pixels than this
WEIGHT_ONE, WEIGHT_MAX = 4096, 16384


def coeff_ksize(in_size, out_size):
    """row length of the (in_size -> out_size) table: 2 * ceil(max(in / out, 1)) + 1"""
    return int(math.ceil(max(in_size / out_size, 1.0))) * 2 + 1


def device_coeffs(in_size, out_size, device):
    """-> (bounds (out_size, 2) int32, kk (out_size, ksize) int32, ksize) on `device`: `resize.pil_bilinear_coeffs(in_size, out_size)` bit
    for bit, built by one launch"""
    _args.integer(in_size, "in_size", 1), _args.integer(out_size, "out_size", 1)
    ksize = coeff_ksize(in_size, out_size)
    bounds = torch.empty((out_size, 2), dtype=torch.int32, device=device)
    kk = torch.empty((out_size, ksize), dtype=torch.int32, device=device)
    L = _lib.check_device(bounds, kk)
    L.call("omni_pil_bilinear_coeffs", in_size, out_size, _lib.ptr(bounds), _lib.ptr(kk), ksize, _lib.stream_of(bounds))
    return bounds, kk, ksize


def crop_resize_u8(img, box, out_h, out_w, flip=False):
    """img (3, H, W) uint8, box = (x0, y0, cw, ch) -> (3, out_h, out_w) uint8 == PIL Image.resize((out_w, out_h), BILINEAR) of
    img[:, y0:y0+ch, x0:x0+cw] followed by an optional horizontal mirror.  Two coefficient launches and the windowed resize."""
    _, H, W = _args.tensor(img, "img", torch.uint8, (3, None, None))
    x0, y0, cw, ch = _args.window(box, H, W)
    _args.integer(out_h, "out_h", 1), _args.integer(out_w, "out_w", 1)
    L = _lib.check_device(img)
    bh, kh, ksh = device_coeffs(cw, out_w, img.device)
    bv, kv, ksv = device_coeffs(ch, out_h, img.device)
    out = _args.empty((3, out_h, out_w), torch.uint8, img)
    tmp = _args.empty((3 * ch * out_w,), torch.uint8, img)
    L.call("omni_crop_resize_u8", _lib.ptr(img), _lib.ptr(out), _lib.ptr(tmp), 3, H, W, x0, y0, ch, cw, out_h, out_w, _lib.ptr(bh),
           _lib.ptr(kh), ksh, _lib.ptr(bv), _lib.ptr(kv), ksv, int(bool(flip)), _lib.stream_of(img))
    return out


def red_plane(fmt):
    if fmt not in ("BGR", "RGB"):
        raise ValueError(f"fmt must be 'BGR' or 'RGB', got {fmt!r}")
    return 2 if fmt == "BGR" else 0


def color_jitter_u8_(img, wb, wc, ws, fmt):
    """brightness wb, contrast wc and saturation ws (integers, 4096 = 1.0, each in [0, 16384]) applied in place to the (3, H, W) uint8
    image `img` in channel order `fmt` ("BGR" or "RGB"), by the integer definition of include/omni3d_hip.h -> img"""
    _, H, W = _args.tensor(img, "img", torch.uint8, (3, None, None))
    for name, w in (("wb", wb), ("wc", wc), ("ws", ws)):
        _args.integer(w, name, 0, WEIGHT_MAX)               # WEIGHT_ONE = 1.0
    c_red = red_plane(fmt)
    if min(H, W) < 1:
        raise ValueError("img must not be empty")
    L = _lib.check_device(img)
    if wb == wc == ws == WEIGHT_ONE:
        return img
    total = _args.empty((1,), torch.int64, img)         # the contrast sum: written and read on the device only
    L.call("omni_color_jitter_u8", _lib.ptr(img), H, W, wb, wc, ws, c_red, _lib.ptr(total), _lib.stream_of(img))
    return img


def warp_denominator_positive(m, out_h, out_w):
    """the third row of the 3 x 3 map `m` is positive at the four corners of the out_h x out_w output rectangle, hence all over it: the
    entry's check, in its arithmetic"""
    m6, m7, m8 = (float(v) for v in m[2])
    return all((m6 * x + m7 * y) + m8 > 0.0 for y in (0.0, float(out_h)) for x in (0.0, float(out_w)))


def warp_homography_u8(img, m, out_h, out_w, fill=(0, 0, 0)):
    """img (3, H, W) uint8 -> a new (3, out_h, out_w) uint8 tensor: output pixel (j + 0.5, i + 0.5) takes the bilinear sample of `img` at
    m @ (j + 0.5, i + 0.5, 1), by the integer definition of include/omni3d_hip.h (omni_warp_homography_u8); where the map leaves the
    source the pixel is `fill`, one byte per plane.  m: 3 x 3 finite numbers with a positive denominator over the output rectangle.
    The matrix and the fill travel in the launch's arguments: one launch, nothing uploaded."""
    _, H, W = _args.tensor(img, "img", torch.uint8, (3, None, None))
    if min(H, W) < 1:
        raise ValueError("img must not be empty")
    m = _args.matrix3(m, "m")
    _args.integer(out_h, "out_h", 1), _args.integer(out_w, "out_w", 1)
    if not isinstance(fill, (tuple, list)) or len(fill) != 3:
        raise ValueError(f"fill must be three integers in [0, 255], got {fill!r}")
    fill = np.array([_args.integer(v, f"fill[{i}]", 0, 255) for i, v in enumerate(fill)], dtype=np.uint8)
    if not warp_denominator_positive(m, out_h, out_w):
        raise ValueError("m must have a positive denominator m[2] @ (x, y, 1) at every corner of the output rectangle")
    L = _lib.check_device(img)
    out = _args.empty((3, out_h, out_w), torch.uint8, img)
    L.call("omni_warp_homography_u8", _lib.ptr(img), _lib.ptr(out), 3, H, W, out_h, out_w, m.ctypes.data, fill.ctypes.data, _lib.stream_of(img))
    return out
