"""omni_crop_resize_u8 (csrc/augment.hip): the PIL-exact resize of a WINDOW of an image, read in place.  The oracle is PIL itself on the
cropped array (then np.flip), bit for bit; every pixel outside the window holds the complement of its nearest pixel inside, so a read
outside the window changes the answer."""
import numpy as np
import pytest
import torch

from ref_augment import pil_resize

CASES = [  # H, W, (x0, y0, cw, ch), HO, WO, flip
    (40, 57, (0, 0, 30, 20), 33, 50, 0),          # top-left corner, upscale
    (40, 57, (27, 20, 30, 20), 9, 13, 1),         # bottom-right corner, antialiased downscale
    # horizontal pass only, odd pitch.  The issue lists this window in a 97-row image, where rows 3..99 do not fit and the entry must
    # refuse it; the image is 100 rows here so that the window as listed, the sizes and the flip stand (it now ends on the last row)
    (100, 131, (5, 3, 60, 97), 97, 41, 1),
    (64, 48, (7, 4, 48 - 7, 50), 31, 41, 0),      # vertical pass only, straight out of the source
    (33, 47, (3, 2, 40, 30), 30, 40, 1),          # mirror only
    (33, 47, (3, 2, 40, 30), 30, 40, 0),          # copy only
    (20, 20, (4, 4, 1, 1), 5, 5, 0),              # one-pixel window
    (900, 1200, (100, 75, 1000, 750), 800, 1067, 1),   # both passes stride over the grid a second, partial time
]


def _source(rs, H, W, box):
    x0, y0, cw, ch = box
    img = rs.randint(0, 256, size=(3, H, W)).astype(np.uint8)
    img[:, y0:y0 + max(ch // 3, 1), x0:x0 + cw] = 255       # saturated and black blocks inside the window: the 8-bit clipping
    img[:, y0:y0 + ch, x0:x0 + max(cw // 4, 1)] = 0
    yy = np.clip(np.arange(H), y0, y0 + ch - 1)[:, None]
    xx = np.clip(np.arange(W), x0, x0 + cw - 1)[None, :]
    poisoned = 255 - img[:, yy, xx]
    inside = np.zeros((H, W), bool)
    inside[y0:y0 + ch, x0:x0 + cw] = True
    return np.where(inside[None], img, poisoned).astype(np.uint8)


def _prefilled(src, box, out_h, out_w, flip):
    """the launch of augment.crop_resize_u8 with the output and the intermediate image pre-filled with 0xFF -> (out, tmp)"""
    from omni3d_amd import lib
    from omni3d_amd.kernels import augment
    _, H, W = src.shape
    x0, y0, cw, ch = box
    bh, kh, ksh = augment.device_coeffs(max(cw, 1), out_w, src.device)
    bv, kv, ksv = augment.device_coeffs(max(ch, 1), out_h, src.device)
    out = torch.full((3, out_h, out_w), 255, dtype=torch.uint8, device=src.device)
    tmp = torch.full((3 * max(ch, 1) * out_w,), 255, dtype=torch.uint8, device=src.device)
    lib.get().call("omni_crop_resize_u8", src.data_ptr(), out.data_ptr(), tmp.data_ptr(), 3, H, W, x0, y0, ch, cw, out_h, out_w,
                   bh.data_ptr(), kh.data_ptr(), ksh, bv.data_ptr(), kv.data_ptr(), ksv, int(flip), lib.stream_of(src))
    return out, tmp


def _run(dev, cases):
    from omni3d_amd.kernels import augment
    rs = np.random.RandomState(0)
    for H, W, box, oh, ow, flip in cases:
        x0, y0, cw, ch = box
        img = _source(rs, H, W, box)
        want = pil_resize(np.ascontiguousarray(img[:, y0:y0 + ch, x0:x0 + cw]), oh, ow, flip)
        src = torch.from_numpy(img).to(dev)
        got = augment.crop_resize_u8(src, box, oh, ow, bool(flip)).cpu().numpy()
        assert got.shape == want.shape
        assert np.array_equal(got, want), (H, W, box, oh, ow, flip, int(np.abs(got.astype(int) - want.astype(int)).max()))
        got = _prefilled(src, box, oh, ow, flip)[0].cpu().numpy()
        assert np.array_equal(got, want), (H, W, box, oh, ow, flip, "0xFF-prefilled output")
        assert np.array_equal(src.cpu().numpy(), img), "the source was written"


def test_large_case_strides_over_the_grid():
    """the last case's two passes have more work items than the launcher's grid has threads, and no multiple of them"""
    from omni3d_amd.kernels.augment import CROP_GRID_THREADS
    H, W, (x0, y0, cw, ch), oh, ow, flip = CASES[-1]
    for n in (3 * ch * ow, 3 * oh * ow):
        assert n > CROP_GRID_THREADS and n % CROP_GRID_THREADS != 0, (n, CROP_GRID_THREADS)


def _full_window(dev):
    from omni3d_amd.kernels import augment, resize
    rs = np.random.RandomState(1)
    for H, W, oh, ow, flip in ((37, 53, 64, 91, True), (120, 160, 48, 64, False), (33, 47, 33, 47, False)):
        src = torch.from_numpy(rs.randint(0, 256, size=(3, H, W)).astype(np.uint8)).to(dev)
        want = resize.resize_bilinear_u8(src, oh, ow, flip)
        got = augment.crop_resize_u8(src, (0, 0, W, H), oh, ow, flip)
        assert torch.equal(got, want), (H, W, oh, ow, flip)


def _rejects(dev):
    """six windows with one defect each: status 1 from the entry, ValueError from the launcher, and the 0xFF-filled output and
    intermediate image untouched -- nothing is launched on rejection"""
    from omni3d_amd import lib
    from omni3d_amd.kernels import augment
    H, W = 40, 57
    src = torch.zeros((3, H, W), dtype=torch.uint8, device=dev)
    bh, kh, ksh = augment.device_coeffs(30, 50, src.device)
    bv, kv, ksv = augment.device_coeffs(20, 33, src.device)
    for x0, y0, cw, ch in ((-1, 0, 30, 20), (0, -1, 30, 20), (28, 0, 30, 20), (0, 21, 30, 20), (0, 0, 0, 20), (0, 0, 30, 0)):
        out = torch.full((3, 33, 50), 255, dtype=torch.uint8, device=dev)
        tmp = torch.full((3 * 20 * 50,), 255, dtype=torch.uint8, device=dev)
        with pytest.raises(lib.OmniHipError, match="status 1"):
            lib.get().call("omni_crop_resize_u8", src.data_ptr(), out.data_ptr(), tmp.data_ptr(), 3, H, W, x0, y0, ch, cw, 33, 50, bh.data_ptr(),
                           kh.data_ptr(), ksh, bv.data_ptr(), kv.data_ptr(), ksv, 0, lib.stream_of(src))
        assert bool((out == 255).all()) and bool((tmp == 255).all()), ("a rejected call wrote", (x0, y0, cw, ch))
        with pytest.raises(ValueError):
            augment.crop_resize_u8(src, (x0, y0, cw, ch), 33, 50)
    for bad in ((0, 0, 30), (0, 0, 30.0, 20), "abcd"):
        with pytest.raises(ValueError):
            augment.crop_resize_u8(src, bad, 33, 50)
    with pytest.raises(ValueError):
        augment.crop_resize_u8(src.float(), (0, 0, 30, 20), 33, 50)
    with pytest.raises(ValueError):
        augment.crop_resize_u8(src, (0, 0, 30, 20), 0, 50)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_crop_resize_matches_pil_emulated(emu_lib, case):
    _run("cpu", [CASES[case]])


def test_full_window_equals_resize_emulated(emu_lib):
    _full_window("cpu")


def test_bad_windows_are_rejected_emulated(emu_lib):
    _rejects("cpu")


@pytest.mark.gpu
def test_crop_resize_matches_pil_gpu(hip_lib):
    _run("cuda", CASES)


@pytest.mark.gpu
def test_full_window_equals_resize_gpu(hip_lib):
    _full_window("cuda")


@pytest.mark.gpu
def test_bad_windows_are_rejected_gpu(hip_lib):
    _rejects("cuda")
