"""omni_warp_homography_u8 (csrc/warp.hip): the projective warp behind INPUT.CAMERA_ROTATION.  Exact cases that need no second
implementation (identity, integer shift, half turn, a window of the source with everything outside it poisoned); general homographies
against the host definition `warp_homography_u8_host`, bit for bit; the host definition against float64 bilinear sampling; the
entry's rejections.  Emulated library and GPU run the same checks."""
import numpy as np
import pytest
import torch

H, W = 120, 160
K0 = np.array([[150.0, 0.0, 83.5], [0.0, 150.0, 57.25], [0.0, 0.0, 1.0]])
FILL = (7, 130, 251)                               # distinct bytes per plane
LARGE = (600, 900)                                 # output of the case that strides over the grid


def _source(rs, h, w):
    """random bytes with a saturated block and a black block"""
    img = rs.randint(0, 256, size=(3, h, w)).astype(np.uint8)
    img[:, : max(h // 3, 1), : max(w // 2, 1)] = 255
    img[:, h // 2:, : max(w // 4, 1)] = 0
    return img


def _hinv(roll, pitch, yaw, K=K0):
    from omni3d_amd.d2.data import camera_rotation, rotation_homography
    return rotation_homography(K, camera_rotation(roll, pitch, yaw))[1]


def _shift(dx, dy):
    return np.array([[1.0, 0.0, dx], [0.0, 1.0, dy], [0.0, 0.0, 1.0]])


def _raw(dev, src, m, oh, ow, fill, out=None):
    """the entry itself; `out` pre-filled by the caller -> out"""
    from omni3d_amd import lib
    out = torch.empty((src.shape[0], oh, ow), dtype=torch.uint8, device=dev) if out is None else out
    mm = np.ascontiguousarray(np.asarray(m, np.float64).reshape(9))
    ff = np.ascontiguousarray(np.asarray(fill, np.uint8))
    lib.get().call("omni_warp_homography_u8", src.data_ptr(), out.data_ptr(), src.shape[0], src.shape[1], src.shape[2], oh, ow, mm.ctypes.data,
                   ff.ctypes.data, lib.stream_of(src))
    return out


# ---- exact cases --------------------------------------------------------------------------------------------------------------------------
def _exact(dev):
    from omni3d_amd.kernels import augment
    rs = np.random.RandomState(0)
    for h, w in ((H, W), (33, 47)):
        img = _source(rs, h, w)
        src = torch.from_numpy(img).to(dev)
        # identity
        got = augment.warp_homography_u8(src, np.eye(3), h, w, FILL).cpu().numpy()
        assert np.array_equal(got, img), "identity"
        # integer shift: output (j, i) reads source (j + 3, i - 2)
        got = augment.warp_homography_u8(src, _shift(3, -2), h, w, FILL).cpu().numpy()
        want = np.empty_like(img)
        want[:] = np.asarray(FILL, np.uint8)[:, None, None]
        want[:, 2:, : w - 3] = img[:, : h - 2, 3:]
        # u = j + 3.5 <= w holds up to column w - 4, v = i - 1.5 >= 0 from row 2 on: the rest is the fill
        assert np.array_equal(got[:, 2:, : w - 3], want[:, 2:, : w - 3]), "shifted copy"
        assert np.array_equal(got[:, :2, :], want[:, :2, :]) and np.array_equal(got[:, :, w - 3:], want[:, :, w - 3:]), "margin is the fill"
        # half turn about the centre
        got = augment.warp_homography_u8(src, [[-1, 0, w], [0, -1, h], [0, 0, 1]], h, w, FILL).cpu().numpy()
        assert np.array_equal(got, np.flip(img, axis=(1, 2))), "180 degree roll"
        assert np.array_equal(src.cpu().numpy(), img), "the source was written"


def _window(dev):
    """HO, WO != H, W with a shift: the output is the window [x0, x0 + cw) x [y0, y0 + ch) of the source.  Every pixel outside the window
    that the map reaches holds the complement of its nearest inside pixel, so a read outside the window changes the answer"""
    from omni3d_amd.kernels import augment
    rs = np.random.RandomState(1)
    for h, w, (x0, y0, cw, ch) in ((H, W, (21, 13, 90, 70)), (33, 47, (3, 2, 40, 30)), (40, 57, (0, 0, 30, 20)), (40, 57, (27, 20, 30, 20))):
        img = _source(rs, h, w)
        yy, xx = np.clip(np.arange(h), y0, y0 + ch - 1)[:, None], np.clip(np.arange(w), x0, x0 + cw - 1)[None, :]
        inside = np.zeros((h, w), bool)
        inside[y0:y0 + ch, x0:x0 + cw] = True
        img = np.where(inside[None], img, 255 - img[:, yy, xx]).astype(np.uint8)
        src = torch.from_numpy(img).to(dev)
        want = img[:, y0:y0 + ch, x0:x0 + cw]
        got = augment.warp_homography_u8(src, _shift(x0, y0), ch, cw, FILL).cpu().numpy()
        assert np.array_equal(got, want), (h, w, x0, y0)
        pre = torch.full((3, ch, cw), 255, dtype=torch.uint8, device=dev)
        assert np.array_equal(_raw(dev, src, _shift(x0, y0), ch, cw, FILL, pre).cpu().numpy(), want), "0xFF-prefilled output"
        assert np.array_equal(src.cpu().numpy(), img), "the source was written"


# ---- general homographies against the host definition ------------------------------------------------------------------------------------
def _cases():
    both = _hinv(5.0, -3.0, 4.0)
    tiny = np.array([[2.0, 0.0, 0.5], [0.0, 2.0, 0.5], [0.0, 0.0, 1.0]])      # a focal length at which these angles move the one pixel by less than itself
    odd = np.array([[40.0, 0.0, 23.0], [0.0, 40.0, 17.0], [0.0, 0.0, 1.0]])
    return [  # name, (h, w), m, (oh, ow)
        ("roll", (H, W), _hinv(5.0, 0.0, 0.0), (H, W)),
        ("pitch", (H, W), _hinv(0.0, -3.0, 0.0), (H, W)),
        ("yaw", (H, W), _hinv(0.0, 0.0, 4.0), (H, W)),
        ("all three", (H, W), both, (H, W)),
        ("all three, crop offset", (H, W), both @ _shift(31, 22), (70, 90)),
        ("1 x 1 source", (1, 1), _hinv(5.0, -3.0, 4.0, tiny) @ np.diag([1.0 / 7, 1.0 / 5, 1.0]), (5, 7)),
        ("1 x 1 output", (H, W), both @ _shift(80, 60), (1, 1)),
        ("odd source", (33, 47), _hinv(5.0, -3.0, 4.0, odd), (33, 47)),
        # more output pixels than the grid has threads: a down-scaling map over the 120 x 160 source, rotated
        ("strides over the grid", (H, W), both @ np.diag([W / LARGE[1], H / LARGE[0], 1.0]), LARGE),
    ]


def test_large_case_strides_over_the_grid():
    """the last case has more output pixels than the launcher's grid has threads, and no multiple of them"""
    from omni3d_amd.kernels.augment import WARP_GRID_THREADS
    n = LARGE[0] * LARGE[1]
    assert _cases()[-1][3] == LARGE and n > WARP_GRID_THREADS and n % WARP_GRID_THREADS != 0, (n, WARP_GRID_THREADS)


def _general(dev, cases):
    from omni3d_amd.cubercnn.data.dataset_mapper import warp_homography_u8_host
    from omni3d_amd.kernels import augment
    rs = np.random.RandomState(2)
    for name, (h, w), m, (oh, ow) in cases:
        img = _source(rs, h, w)
        want = warp_homography_u8_host(img, m, oh, ow, FILL)
        src = torch.from_numpy(img).to(dev)
        got = augment.warp_homography_u8(src, m, oh, ow, FILL).cpu().numpy()
        assert got.shape == want.shape == (3, oh, ow)
        diff = got.astype(int) - want.astype(int)
        assert np.array_equal(got, want), (name, int(np.count_nonzero(diff)), int(np.abs(diff).max()))
        filled = (want == np.asarray(FILL, np.uint8)[:, None, None]).all(axis=0)
        assert not filled.all(), (name, "the case shows nothing of the image")
        assert filled.any() or (oh, ow) != (h, w), (name, "a rotated full frame shows some border")
        assert np.array_equal(src.cpu().numpy(), img), "the source was written"


# ---- the host definition against float64 bilinear sampling (CPU only) --------------------------------------------------------------------
def test_host_definition_is_a_bilinear_warp():
    """truth: float64 bilinear sampling at the same (su, sv) with the same edge rule.  The weights are rounded to 1/256, an error of at
    most 1/512 each, hence at most 2 * 255 / 512 < 1.0 in the value; the final rounding adds 0.5: |out - exact| <= 1.5"""
    from omni3d_amd.cubercnn.data.dataset_mapper import warp_homography_u8_host
    rs = np.random.RandomState(3)
    seen = 0
    for name, (h, w), m, (oh, ow) in _cases():
        img = _source(rs, h, w)
        out = warp_homography_u8_host(img, m, oh, ow, FILL).astype(np.float64)
        mm = np.asarray(m, np.float64).reshape(9)
        xd, yd = (np.arange(ow) + 0.5)[None, :], (np.arange(oh) + 0.5)[:, None]
        D = mm[6] * xd + mm[7] * yd + mm[8]
        u, v = (mm[0] * xd + mm[1] * yd + mm[2]) / D, (mm[3] * xd + mm[4] * yd + mm[5]) / D
        # pixels both call inside: a margin of 1e-9 keeps those on the border line, where rounding decides, out of the comparison
        inside = (u >= 1e-9) & (u <= w - 1e-9) & (v >= 1e-9) & (v <= h - 1e-9)
        su, sv = np.where(inside, u, 0.5) - 0.5, np.where(inside, v, 0.5) - 0.5
        fx, fy = np.floor(su), np.floor(sv)
        ax, ay = su - fx, sv - fy
        x0, y0 = fx.astype(int), fy.astype(int)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        x0, y0 = np.maximum(x0, 0), np.maximum(y0, 0)
        s = img.astype(np.float64)
        exact = (s[:, y0, x0] * (1 - ax) + s[:, y0, x1] * ax) * (1 - ay) + (s[:, y1, x0] * (1 - ax) + s[:, y1, x1] * ax) * ay
        err = np.abs(out - exact)[:, inside]
        seen += err.size
        assert err.size == 0 or err.max() <= 1.5, (name, float(err.max()))
    assert seen > 100000


# ---- rejections ---------------------------------------------------------------------------------------------------------------------------
def _rejects(dev):
    """one defect each: status 1 from the entry, the 0xFF-filled output untouched, ValueError from the launcher"""
    from omni3d_amd import lib
    from omni3d_amd.kernels import augment
    src = torch.zeros((3, 40, 57), dtype=torch.uint8, device=dev)
    five = torch.zeros((5, 40, 57), dtype=torch.uint8, device=dev)
    eye = np.eye(3)
    m = np.ascontiguousarray(eye.reshape(9))
    fill = np.zeros(5, np.uint8)
    out = torch.full((5, 33, 50), 255, dtype=torch.uint8, device=dev)
    call = lambda *a: lib.get().call("omni_warp_homography_u8", *a, lib.stream_of(src))      # noqa: E731
    S, O, M, F = src.data_ptr(), out.data_ptr(), m.ctypes.data, fill.ctypes.data

    def mat(**kw):
        a = eye.copy().reshape(9)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return np.ascontiguousarray(a)
    nan, inf = mat(m4=float("nan")), mat(m2=float("inf"))
    neg = mat(m6=-1.0 / 40.0)                      # D = 1 - x / 40: negative at x = 50
    zero = mat(m7=-1.0 / 32.0)                     # D = 1 - y / 32: exactly 0 at the corner y = 32 of a 32-row output
    bad = {
        "null src": (None, O, 3, 40, 57, 33, 50, M, F), "null dst": (S, None, 3, 40, 57, 33, 50, M, F),
        "null m": (S, O, 3, 40, 57, 33, 50, None, F), "null fill": (S, O, 3, 40, 57, 33, 50, M, None),
        "planes 0": (S, O, 0, 40, 57, 33, 50, M, F), "H 0": (S, O, 3, 0, 57, 33, 50, M, F), "W 0": (S, O, 3, 40, 0, 33, 50, M, F),
        "HO 0": (S, O, 3, 40, 57, 0, 50, M, F), "WO 0": (S, O, 3, 40, 57, 33, 0, M, F),
        "planes 5": (five.data_ptr(), O, 5, 40, 57, 33, 50, M, F),
        "nan": (S, O, 3, 40, 57, 33, 50, nan.ctypes.data, F), "inf": (S, O, 3, 40, 57, 33, 50, inf.ctypes.data, F),
        "D < 0": (S, O, 3, 40, 57, 33, 50, neg.ctypes.data, F), "D = 0": (S, O, 3, 40, 57, 32, 50, zero.ctypes.data, F),
    }
    for name, args in bad.items():
        with pytest.raises(lib.OmniHipError, match="status 1"):
            call(*args)
        assert bool((out == 255).all()), ("a rejected call wrote", name)
    # dst inside src: a (3, 10, 10) output that starts in the second row of a 0xFF-filled source
    big = torch.full((3, 40, 57), 255, dtype=torch.uint8, device=dev)
    with pytest.raises(lib.OmniHipError, match="status 1"):
        call(big.data_ptr(), big.data_ptr() + 57, 3, 40, 57, 10, 10, M, F)
    assert bool((big == 255).all()), "a rejected call wrote"
    for m_bad, oh in ((nan, 33), (inf, 33), (neg, 33), (zero, 32), (np.zeros(6), 33), ("abc", 33), (None, 33)):
        with pytest.raises(ValueError):
            augment.warp_homography_u8(src, m_bad.reshape(-1, 3) if isinstance(m_bad, np.ndarray) else m_bad, oh, 50)
    assert augment.warp_homography_u8(src, zero.reshape(3, 3), 31, 50).shape == (3, 31, 50), "D > 0 all over a 31-row output"
    for h, w in ((0, 50), (33, 0), (33.0, 50)):
        with pytest.raises(ValueError):
            augment.warp_homography_u8(src, eye, h, w)
    for t in (src.float(), src[0], five, src[:, :, ::2], torch.zeros((3, 0, 57), dtype=torch.uint8, device=dev)):
        with pytest.raises(ValueError):
            augment.warp_homography_u8(t, eye, 33, 50)
    for f in ((0, 0), (0, 0, 256), (0, -1, 0), (0.0, 0, 0), "abc"):
        with pytest.raises(ValueError):
            augment.warp_homography_u8(src, eye, 33, 50, f)


def test_exact_cases_emulated(emu_lib):
    _exact("cpu")


def test_window_reads_nothing_outside_emulated(emu_lib):
    _window("cpu")


@pytest.mark.parametrize("case", range(9))
def test_matches_host_definition_emulated(emu_lib, case):
    _general("cpu", [_cases()[case]])


def test_rejections_emulated(emu_lib):
    _rejects("cpu")


@pytest.mark.gpu
def test_exact_cases_gpu(hip_lib):
    _exact("cuda")


@pytest.mark.gpu
def test_window_reads_nothing_outside_gpu(hip_lib):
    _window("cuda")


@pytest.mark.gpu
def test_matches_host_definition_gpu(hip_lib):
    _general("cuda", _cases())


@pytest.mark.gpu
def test_rejections_gpu(hip_lib):
    _rejects("cuda")
