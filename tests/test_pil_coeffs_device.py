"""omni_pil_bilinear_coeffs (csrc/augment.hip): Pillow's coefficient rows built on the device are bit-equal to the host construction
`kernels/resize.py::pil_bilinear_coeffs`, which tests/test_resize.py pins to PIL itself."""
import numpy as np
import pytest
import torch

PAIRS = [(1, 1), (1, 7), (7, 1), (2, 3), (53, 91), (160, 64), (131, 60), (1000, 1067), (1242, 640), (4093, 257), (97, 97)]


def _tables(dev, in_size, out_size):
    """the launch of augment.device_coeffs with both tables pre-filled with 0xFF: an unwritten zero of a row's tail would show"""
    from omni3d_amd import lib
    from omni3d_amd.kernels import augment
    ksize = augment.coeff_ksize(in_size, out_size)
    bounds = torch.full((out_size, 2), -1, dtype=torch.int32, device=dev)
    kk = torch.full((out_size, ksize), -1, dtype=torch.int32, device=dev)
    lib.get().call("omni_pil_bilinear_coeffs", in_size, out_size, bounds.data_ptr(), kk.data_ptr(), ksize, lib.stream_of(bounds))
    return bounds.cpu().numpy(), kk.cpu().numpy(), ksize


def _run(dev):
    from omni3d_amd.kernels import augment
    from omni3d_amd.kernels.resize import pil_bilinear_coeffs
    for in_size, out_size in PAIRS:
        want_b, want_k, want_ks = pil_bilinear_coeffs(in_size, out_size)
        got_b, got_k, ks = _tables(dev, in_size, out_size)
        assert ks == want_ks, (in_size, out_size)
        assert np.array_equal(got_b, want_b), (in_size, out_size, "bounds")
        assert np.array_equal(got_k, want_k), (in_size, out_size, "kk", int(np.abs(got_k.astype(np.int64) - want_k).max()))
        b, k, ks = augment.device_coeffs(in_size, out_size, dev)
        assert ks == want_ks and b.dtype == k.dtype == torch.int32 and b.device.type == torch.device(dev).type
        assert np.array_equal(b.cpu().numpy(), want_b) and np.array_equal(k.cpu().numpy(), want_k), (in_size, out_size, "launcher")


def _rejects(dev):
    from omni3d_amd import lib
    from omni3d_amd.kernels import augment
    bounds = torch.full((64, 2), -1, dtype=torch.int32, device=dev)
    kk = torch.full((64, 9), -1, dtype=torch.int32, device=dev)
    st = lib.stream_of(bounds)
    assert augment.coeff_ksize(160, 64) == 7
    for in_size, out_size, ksize in ((160, 64, 5), (160, 64, 9), (160, 64, 0), (0, 64, 3), (160, 0, 3), (-1, 64, 3)):
        with pytest.raises(lib.OmniHipError, match="status 1"):
            lib.get().call("omni_pil_bilinear_coeffs", in_size, out_size, bounds.data_ptr(), kk.data_ptr(), ksize, st)
    with pytest.raises(lib.OmniHipError, match="status 1"):
        lib.get().call("omni_pil_bilinear_coeffs", 160, 64, None, kk.data_ptr(), 7, st)
    assert bool((bounds == -1).all()) and bool((kk == -1).all()), "a rejected call wrote"
    for bad in ((0, 4), (4, 0), (4.0, 4), (True, 4)):
        with pytest.raises(ValueError):
            augment.device_coeffs(bad[0], bad[1], dev)


def test_device_coefficients_equal_the_host_tables_emulated(emu_lib):
    _run("cpu")


def test_wrong_ksize_is_rejected_emulated(emu_lib):
    _rejects("cpu")


@pytest.mark.gpu
def test_device_coefficients_equal_the_host_tables_gpu(hip_lib):
    _run("cuda")


@pytest.mark.gpu
def test_wrong_ksize_is_rejected_gpu(hip_lib):
    _rejects("cuda")
