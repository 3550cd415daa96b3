"""References of the augmentation tests, written from the definitions in include/omni3d_hip.h and DESIGN.md, not from the kernels:
the integer colour jitter in numpy int64, detectron2's RandomCrop sampling, and the pinhole projection in float64."""
import numpy as np


def weight(w):
    """a float weight as the 12-fractional-bit integer the kernels take"""
    return int(w * 4096 + 0.5)


def color_jitter(img, wb, wc, ws, c_red):
    """img (3, H, W) uint8, integer weights, c_red = plane of red (0 RGB / 2 BGR) -> (3, H, W) uint8"""
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[0] == 3 and c_red in (0, 2)
    v = img.astype(np.int64)
    v1 = np.clip((wb * v + 2048) >> 12, 0, 255)
    S, N = int(v1.sum()), int(v1.size)
    M8 = (256 * S + N // 2) // N
    v2 = np.clip((wc * 256 * v1 + (4096 - wc) * M8 + (1 << 19)) >> 20, 0, 255)
    R2, G2, B2 = v2[c_red], v2[1], v2[2 - c_red]
    g8 = 77 * R2 + 150 * G2 + 29 * B2
    v3 = np.clip((ws * 256 * v2 + (4096 - ws) * g8[None, :, :] + (1 << 19)) >> 20, 0, 255)
    return v3.astype(np.uint8)


def crop_box(h, w, crop_type, crop_size, rng):
    """detectron2 RandomCrop: get_crop_size, then the origin (row first) -> (x0, y0, cw, ch)"""
    if crop_type == "relative":
        croph, cropw = int(h * crop_size[0] + 0.5), int(w * crop_size[1] + 0.5)
    elif crop_type == "relative_range":
        size = np.asarray(crop_size, dtype=np.float32)
        frac = size + rng.rand(2) * (1 - size)
        croph, cropw = int(h * frac[0] + 0.5), int(w * frac[1] + 0.5)
    elif crop_type == "absolute":
        croph, cropw = min(crop_size[0], h), min(crop_size[1], w)
    else:
        assert crop_type == "absolute_range"
        croph = rng.randint(min(h, crop_size[0]), min(h, crop_size[1]) + 1)
        cropw = rng.randint(min(w, crop_size[0]), min(w, crop_size[1]) + 1)
    y0 = rng.randint(h - croph + 1)
    x0 = rng.randint(w - cropw + 1)
    return x0, y0, cropw, croph


def project(K, pts):
    """K (3, 3), pts (n, 3) camera coordinates -> (n, 2) pixels, float64"""
    K, pts = np.asarray(K, np.float64), np.asarray(pts, np.float64).reshape(-1, 3)
    uvw = pts @ K.T
    return uvw[:, :2] / uvw[:, 2:3]


def pil_resize(img_chw, out_h, out_w, flip):
    from PIL import Image
    hwc = np.ascontiguousarray(img_chw.transpose(1, 2, 0))
    out = np.asarray(Image.fromarray(hwc).resize((out_w, out_h), Image.BILINEAR))
    if flip:
        out = np.flip(out, axis=1)
    return np.ascontiguousarray(out.transpose(2, 0, 1))
