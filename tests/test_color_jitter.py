"""omni_color_jitter_u8 (csrc/augment.hip): the integer brightness / contrast / saturation jitter against its definition in numpy int64
(tests/ref_augment.py), bit for bit.  Every image holds a zero block and a 255 block so that both clamps fire."""
import numpy as np
import pytest
import torch

import ref_augment as ref

SHAPES = [(1, 1), (7, 13), (64, 65)]
BIG = (837, 839)                     # more pixels than the apply launch has threads, and no multiple of them; the sum pass likewise
WEIGHTS = [(0.5, 1, 1), (1.7, 1, 1), (1, 0.5, 1), (1, 1.7, 1), (1, 1, 0.5), (1, 1, 1.7),      # each step alone
           (0.8, 1.3, 0.6), (1.25, 0.7, 1.9),                                                # all three together
           (0, 1.3, 0.7), (4.0, 4.0, 4.0)]
BIG_WEIGHTS = [(0.8, 1.3, 0.6), (1, 1, 1.7), (4.0, 4.0, 4.0)]                                # every kernel path, kept short for the emulator


def _image(rs, H, W):
    img = rs.randint(0, 256, size=(3, H, W)).astype(np.uint8)
    img[:, : H // 3, : W // 2] = 0
    img[:, H - H // 3:, W - W // 2:] = 255
    return img


def _jitter(dev, img, w, fmt):
    from omni3d_amd.kernels import augment
    t = torch.from_numpy(img.copy()).to(dev)
    out = augment.color_jitter_u8_(t, *(ref.weight(x) for x in w), fmt)
    assert out is t
    return t.cpu().numpy()


def _check(dev, img, w, what):
    for fmt, c_red in (("BGR", 2), ("RGB", 0)):
        want = ref.color_jitter(img, *(ref.weight(x) for x in w), c_red)
        got = _jitter(dev, img, w, fmt)
        assert np.array_equal(got, want), (what, img.shape, w, fmt, int(np.abs(got.astype(int) - want.astype(int)).max()))
    # a BGR image and its plane-reversed RGB twin give plane-reversed results
    assert np.array_equal(_jitter(dev, img, w, "BGR"), _jitter(dev, np.ascontiguousarray(img[::-1]), w, "RGB")[::-1]), (what, w)


def _run(dev):
    rs = np.random.RandomState(0)
    for H, W in SHAPES:
        img = _image(rs, H, W)
        for w in WEIGHTS:
            _check(dev, img, w, "small")
    a, b = _jitter(dev, img, WEIGHTS[6], "BGR"), _jitter(dev, img, WEIGHTS[6], "BGR")
    assert np.array_equal(a, b), "two runs differ"


def _run_big(dev):
    img = _image(np.random.RandomState(1), *BIG)
    for w in BIG_WEIGHTS:
        _check(dev, img, w, "big")


def test_big_shape_strides_over_the_grid():
    from omni3d_amd.kernels.augment import JITTER_GRID_THREADS
    n = BIG[0] * BIG[1]
    assert n > JITTER_GRID_THREADS and n % JITTER_GRID_THREADS != 0
    assert (3 * n) // 4 > JITTER_GRID_THREADS and ((3 * n) // 4) % JITTER_GRID_THREADS != 0      # the sum pass, four bytes per item


def _identity(dev):
    """all three weights at 4096: the bytes are untouched and the sum cell keeps its sentinel (it is not zeroed).  That no kernel is
    launched is NOT observable here: an apply pass at these weights is the identity by the arithmetic and the emulator counts no
    launches; the entry's early return is read in csrc/augment.hip, not tested."""
    from omni3d_amd import lib
    from omni3d_amd.kernels import augment
    img = _image(np.random.RandomState(2), 7, 13)
    assert np.array_equal(_jitter(dev, img, (1, 1, 1), "BGR"), img)
    t = torch.from_numpy(img.copy()).to(dev)
    cell = torch.full((1,), -7, dtype=torch.int64, device=dev)
    lib.get().call("omni_color_jitter_u8", t.data_ptr(), 7, 13, 4096, 4096, 4096, 2, cell.data_ptr(), lib.stream_of(t))
    assert int(cell) == -7 and np.array_equal(t.cpu().numpy(), img)
    # a step at 4096 is the identity by the arithmetic: brightness + saturation only leave the sum cell alone as well
    lib.get().call("omni_color_jitter_u8", t.data_ptr(), 7, 13, 2048, 4096, 6000, 2, cell.data_ptr(), lib.stream_of(t))
    assert int(cell) == -7 and np.array_equal(t.cpu().numpy(), ref.color_jitter(img, 2048, 4096, 6000, 2))
    assert augment.WEIGHT_ONE == ref.weight(1.0) == 4096


def _unaligned(dev):
    """views at byte offsets 1, 2 and 3 of a larger buffer: the sum pass reads a head of 3, 2 and 1 bytes in front of its first aligned
    dword, then dwords, then a tail; the bytes around the view stay as they were"""
    from omni3d_amd.kernels import augment
    rs = np.random.RandomState(4)
    for H, W in ((1, 1), (7, 13), (64, 65)):
        img = _image(rs, H, W)
        n = img.size
        for off in (1, 2, 3):
            buf = torch.full((n + 8,), 0x5A, dtype=torch.uint8, device=dev)
            assert buf.data_ptr() % 4 == 0
            view = buf[off:off + n].view(3, H, W)
            view.copy_(torch.from_numpy(img))
            assert view.data_ptr() % 4 == off and view.is_contiguous()
            augment.color_jitter_u8_(view, ref.weight(0.8), ref.weight(1.3), ref.weight(0.6), "BGR")
            got = buf.cpu().numpy()
            assert np.array_equal(got[off:off + n].reshape(3, H, W), ref.color_jitter(img, ref.weight(0.8), ref.weight(1.3), ref.weight(0.6), 2)), (H, W, off)
            assert (got[:off] == 0x5A).all() and (got[off + n:] == 0x5A).all(), "bytes outside the view were written"


def _sum_64bit(dev):
    """255 * N = 4 406 400 000 > 2^32: a sum that wrapped at 32 bits gives a mean below 255 and darkens the image"""
    from omni3d_amd.kernels import augment
    t = torch.full((3, 2400, 2400), 255, dtype=torch.uint8, device=dev)
    assert 255 * t.numel() > 2 ** 32
    augment.color_jitter_u8_(t, 4096, 2048, 4096, "BGR")
    assert bool((t == 255).all())


def _rejects(dev):
    from omni3d_amd import lib
    from omni3d_amd.kernels import augment
    img = _image(np.random.RandomState(3), 7, 13)
    t = torch.from_numpy(img.copy()).to(dev)
    cell = torch.full((1,), -7, dtype=torch.int64, device=dev)
    for wb, wc, ws, c_red in ((-1, 4096, 4096, 2), (16385, 4096, 4096, 2), (4096, -1, 4096, 0), (4096, 16385, 4096, 0), (4096, 4096, -1, 2),
                              (4096, 4096, 16385, 2), (2048, 2048, 2048, 1), (2048, 2048, 2048, 3)):
        with pytest.raises(lib.OmniHipError, match="status 1"):
            lib.get().call("omni_color_jitter_u8", t.data_ptr(), 7, 13, wb, wc, ws, c_red, cell.data_ptr(), lib.stream_of(t))
    with pytest.raises(lib.OmniHipError, match="status 1"):
        lib.get().call("omni_color_jitter_u8", t.data_ptr(), 0, 13, 2048, 2048, 2048, 2, cell.data_ptr(), lib.stream_of(t))
    assert int(cell) == -7 and np.array_equal(t.cpu().numpy(), img), "a rejected call wrote"
    for bad in ((-1, 4096, 4096), (4096, 16385, 4096), (4096, 4096, 1.0), (True, 4096, 4096)):
        with pytest.raises(ValueError):
            augment.color_jitter_u8_(t, *bad, "BGR")
    with pytest.raises(ValueError):
        augment.color_jitter_u8_(t, 2048, 2048, 2048, "GBR")
    with pytest.raises(ValueError):
        augment.color_jitter_u8_(t[:2], 2048, 2048, 2048, "BGR")
    assert np.array_equal(t.cpu().numpy(), img)


def test_color_jitter_matches_the_integer_definition_emulated(emu_lib):
    _run("cpu")


def test_color_jitter_big_shape_emulated(emu_lib):
    _run_big("cpu")


def test_identity_weights_leave_bytes_and_sum_cell_emulated(emu_lib):
    _identity("cpu")


def test_unaligned_views_emulated(emu_lib):
    _unaligned("cpu")


def test_contrast_sum_is_64_bit_emulated(emu_lib):
    _sum_64bit("cpu")


def test_out_of_range_weights_are_rejected_emulated(emu_lib):
    _rejects("cpu")


@pytest.mark.gpu
def test_color_jitter_matches_the_integer_definition_gpu(hip_lib):
    _run("cuda")
    _run_big("cuda")


@pytest.mark.gpu
def test_identity_weights_leave_bytes_and_sum_cell_gpu(hip_lib):
    _identity("cuda")


@pytest.mark.gpu
def test_unaligned_views_gpu(hip_lib):
    _unaligned("cuda")


@pytest.mark.gpu
def test_contrast_sum_is_64_bit_gpu(hip_lib):
    _sum_64bit("cuda")


@pytest.mark.gpu
def test_out_of_range_weights_are_rejected_gpu(hip_lib):
    _rejects("cuda")
