"""The memory-bound layer kernels -- csrc/bn_pool.hip below its BatchNorm section, csrc/pool3.hip, csrc/depthwise.hip -- against the
float64 references of tests/ref_layers.py, through the C ABI (include/omni3d_hip.h), at the shapes where their loops engage.

Every output buffer is supplied here and pre-filled with NaN (tests/test_resize.py does the same with 0xFF for the uint8 kernels of
csrc/resize.hip), so an element a kernel never writes is seen.  Every
case runs on two input sets: small integers in [-2, 2] (every partial sum is an integer below 2^24, so fp32 is exact in any order,
atomics included: torch.equal) and normal random values (selecting / moving kernels: torch.equal; adding kernels: error / bound <= 1
with the a-priori bound gamma(L) * sum |terms| of ref_layers.py).  One 'large' case per kernel asserts that its grid-stride loop runs
at least two uneven trips under the launcher's grid cap; the small edge sets run 2x2 / 2x3 / extent-1 inputs, N = 0 and C = 4.

The emulated twins of the large cases take a second or two each, so every case runs in both halves."""
import ctypes

import pytest
import torch

import ref_layers as R
from ref_winograd import worst_ratio

KINDS = ["int", "randn"]
NAN = float("nan")


# ---- plumbing ------------------------------------------------------------------------------------------------------------------
def _call(name, *args):
    """omni3d_amd.lib.get().call(name, ...): tensors become their addresses, the stream of the first tensor is appended"""
    from omni3d_amd import lib
    first = next(a for a in args if isinstance(a, torch.Tensor))
    lib.get().call(name, *[lib.ptr(a) if isinstance(a, torch.Tensor) or a is None else a for a in args], lib.stream_of(first))


def _vals(kind, shape, seed, dev):
    g = torch.Generator().manual_seed(seed)
    if kind == "int":
        return torch.randint(-2, 3, shape, generator=g).float().to(dev)
    return torch.randn(shape, generator=g).to(dev)


def _nan(shape, dev):
    return torch.full(shape, NAN, dtype=torch.float32, device=dev)


def _in_slice(t, lead=8, tail=4):
    """the values of t (..., C) as the channel slice [lead : lead + C] of a wider tensor whose other channels are NaN -> (view, pitch)"""
    C = t.shape[-1]
    wide = torch.full((*t.shape[:-1], lead + C + tail), NAN, dtype=torch.float32, device=t.device)
    wide[..., lead:lead + C] = t
    return wide[..., lead:lead + C], lead + C + tail


def _carry(kind, shape, seed, dev, sliced):
    c = _vals(kind, shape, seed, dev)
    return _in_slice(c) if sliced else (c, shape[-1])


def _same(got, ref64):
    assert got.dtype == torch.float32 and torch.equal(got, ref64.float())


def _close(got, ref64, kind, bound):
    """integers: exact; random values: |got - ref64| <= bound element by element"""
    assert got.shape == ref64.shape and not torch.isnan(got).any()
    if kind == "int" or got.numel() == 0:
        _same(got, ref64)
    else:
        assert worst_ratio(got, ref64, bound) <= 1.0


def _raises(name, *args):
    from omni3d_amd.lib import OmniHipError
    with pytest.raises(OmniHipError):
        _call(name, *args)


# (N, H, W, C): 2x2, 2x3, 3x2, odd extents with C/4 = 3, N = 0
SMALL_POOL2 = [(1, 2, 2, 4), (2, 2, 3, 8), (1, 3, 2, 4), (2, 5, 7, 12), (2, 6, 4, 8), (0, 4, 4, 4)]
SMALL_EVEN = [(1, 2, 2, 4), (2, 2, 4, 8), (2, 6, 10, 12), (0, 4, 4, 4)]
SMALL_ANY = SMALL_POOL2 + [(1, 1, 1, 4), (2, 1, 5, 8), (1, 4, 1, 4)]
LARGE_ODD = (3, 211, 419, 40)       # 3 * 105 * 209 * 10 = 658 350 windows x quads; 667 800 outputs of the stride-2 kernels; 2 652 270 inputs
LARGE_EVEN = (3, 212, 420, 40)      # the carry form of the 2x2 max-pool backward needs even extents: 667 800 windows x quads
LARGE_FPN = (3, 420, 420, 24)       # 3 175 200 pixels x quads, 793 800 for the backward


def _cases(small, large):
    return [(c, False) for c in small] + [(large, True)]


def _ids(case):
    return "x".join(str(v) for v in case[0]) + ("-large" if case[1] else "")


# ---- 2x2 max-pool ----------------------------------------------------------------------------------------------------------------
def _run_maxpool2(dev, kind, case):
    (N, H, W, C), large = case
    if large:
        R.assert_two_uneven_trips(R.items_pool2(N, H, W, C), R.EW_CAP, C)
        assert H % 2 == 1 and W % 2 == 1        # the forward drops the last row and column, the backward zero-fills them
    x, dy = _vals(kind, (N, H, W, C), 1, dev), _vals(kind, (N, H // 2, W // 2, C), 2, dev)
    y = _nan(dy.shape, dev)
    _call("omni_maxpool2_fwd", x, y, N, H, W, C)
    _same(y, R.maxpool2_fwd(x))
    dx = _nan(x.shape, dev)
    _call("omni_maxpool2_bwd", x, dy, dx, N, H, W, C)
    _same(dx, R.maxpool2_bwd(x, dy))
    dys, lddy = _in_slice(dy)                   # pitched dy without a carry (odd extents allowed)
    dx = _nan(x.shape, dev)
    _call("omni_maxpool2_bwd_carry", x, dys, lddy, None, 0, dx, N, H, W, C)
    _same(dx, R.maxpool2_bwd(x, dy))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", _cases(SMALL_POOL2, LARGE_ODD), ids=_ids)
def test_maxpool2_emulated(emu_lib, kind, case):
    _run_maxpool2("cpu", kind, case)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", _cases(SMALL_POOL2, LARGE_ODD), ids=_ids)
def test_maxpool2_gpu(hip_lib, kind, case):
    _run_maxpool2("cuda", kind, case)


def _run_maxpool2_carry(dev, kind, case, dy_sliced, carry_sliced):
    """dx = routed dy + carry against the float64 routing plus the carry (one rounding), dense and as channel slices"""
    (N, H, W, C), large = case
    if large:
        R.assert_two_uneven_trips(R.items_pool2(N, H, W, C), R.EW_CAP, C)
    x, dy = _vals(kind, (N, H, W, C), 3, dev), _vals(kind, (N, H // 2, W // 2, C), 4, dev)
    dyk, lddy = _in_slice(dy) if dy_sliced else (dy, C)
    carry, ldc = _carry(kind, (N, H, W, C), 5, dev, carry_sliced)
    dx = _nan(x.shape, dev)
    _call("omni_maxpool2_bwd_carry", x, dyk, lddy, carry, ldc, dx, N, H, W, C)
    ref = R.maxpool2_bwd(x, dy) + carry.double()
    _close(dx, ref, kind, R.gamma(R.CARRY_CHAIN) * (R.maxpool2_bwd(x, dy, absolute=True) + carry.double().abs()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dy_sliced,carry_sliced", [(False, False), (False, True), (True, True)])
@pytest.mark.parametrize("case", _cases(SMALL_EVEN, LARGE_EVEN), ids=_ids)
def test_maxpool2_bwd_carry_emulated(emu_lib, kind, case, dy_sliced, carry_sliced):
    _run_maxpool2_carry("cpu", kind, case, dy_sliced, carry_sliced)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dy_sliced,carry_sliced", [(False, False), (False, True), (True, True)])
@pytest.mark.parametrize("case", _cases(SMALL_EVEN, LARGE_EVEN), ids=_ids)
def test_maxpool2_bwd_carry_gpu(hip_lib, kind, case, dy_sliced, carry_sliced):
    _run_maxpool2_carry("cuda", kind, case, dy_sliced, carry_sliced)


# ---- 2x2 average pool ------------------------------------------------------------------------------------------------------------
def _run_avgpool2(dev, kind, case):
    (N, H, W, C), large = case
    if large:
        R.assert_two_uneven_trips(R.items_pool2(N, H, W, C), R.EW_CAP, C)
        assert H % 2 == 1 and W % 2 == 1
    x, dy = _vals(kind, (N, H, W, C), 6, dev), _vals(kind, (N, H // 2, W // 2, C), 7, dev)
    y = _nan(dy.shape, dev)
    _call("omni_avgpool2_fwd", x, y, N, H, W, C)
    _close(y, R.avgpool2_fwd(x), kind, R.gamma(R.AVGPOOL_CHAIN) * R.avgpool2_fwd(x, absolute=True))
    dx = _nan(x.shape, dev)
    _call("omni_avgpool2_bwd", dy, dx, N, H, W, C)
    _same(dx, R.avgpool2_bwd(dy, H, W))         # dy / 4 is exact


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", _cases(SMALL_POOL2, LARGE_ODD), ids=_ids)
def test_avgpool2_emulated(emu_lib, kind, case):
    _run_avgpool2("cpu", kind, case)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", _cases(SMALL_POOL2, LARGE_ODD), ids=_ids)
def test_avgpool2_gpu(hip_lib, kind, case):
    _run_avgpool2("cuda", kind, case)


# ---- stride-2 subsample ----------------------------------------------------------------------------------------------------------
def _run_subsample2(dev, kind, case, carry_sliced):
    (N, H, W, C), large = case
    OH, OW = R.out_hw(H, W)
    if large:
        R.assert_two_uneven_trips(R.items_sub(N, H, W, C), R.EW_CAP, C)
        R.assert_two_uneven_trips(R.items_full(N, H, W, C), R.EW_CAP, C)       # the carry form walks the inputs
    x, dy = _vals(kind, (N, H, W, C), 8, dev), _vals(kind, (N, OH, OW, C), 9, dev)
    y = _nan(dy.shape, dev)
    _call("omni_subsample2_fwd", x, y, N, H, W, C)
    _same(y, R.subsample2_fwd(x))
    dx = _nan(x.shape, dev)
    _call("omni_subsample2_bwd", dy, dx, N, H, W, C)
    _same(dx, R.subsample2_bwd(dy, H, W))
    if N == 0:
        return              # (the carry form requires a carry, and an empty tensor has no address)
    carry, ldc = _carry(kind, (N, H, W, C), 10, dev, carry_sliced)
    dx = _nan(x.shape, dev)
    _call("omni_subsample2_bwd_carry", dy, carry, ldc, dx, N, H, W, C)
    ref = R.subsample2_bwd(dy, H, W) + carry.double()
    _close(dx, ref, kind, R.gamma(R.CARRY_CHAIN) * (R.subsample2_bwd(dy, H, W, absolute=True) + carry.double().abs()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("carry_sliced", [False, True])
@pytest.mark.parametrize("case", _cases(SMALL_ANY, LARGE_ODD), ids=_ids)
def test_subsample2_emulated(emu_lib, kind, case, carry_sliced):
    _run_subsample2("cpu", kind, case, carry_sliced)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("carry_sliced", [False, True])
@pytest.mark.parametrize("case", _cases(SMALL_ANY, LARGE_ODD), ids=_ids)
def test_subsample2_gpu(hip_lib, kind, case, carry_sliced):
    _run_subsample2("cuda", kind, case, carry_sliced)


# ---- 3x3 / stride 2 / padding 1 max-pool -------------------------------------------------------------------------------------------
def _run_maxpool3(dev, kind, case):
    (N, H, W, C), large = case
    OH, OW = R.out_hw(H, W)
    if large:
        R.assert_two_uneven_trips(R.items_sub(N, H, W, C), R.EW_CAP, C)
        R.assert_two_uneven_trips(R.items_full(N, H, W, C), R.EW_CAP, C)
    x, dy = _vals(kind, (N, H, W, C), 11, dev), _vals(kind, (N, OH, OW, C), 12, dev)
    y = _nan(dy.shape, dev)
    _call("omni_maxpool3s2_fwd", x, y, N, H, W, C)
    _same(y, R.maxpool3s2_fwd(x))
    dx = _nan(x.shape, dev)
    _call("omni_maxpool3s2_bwd", x, dy, dx, N, H, W, C)
    _close(dx, R.maxpool3s2_bwd(x, dy), kind, R.gamma(R.MAXPOOL3_BWD_CHAIN) * R.maxpool3s2_bwd(x, dy, absolute=True))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", _cases(SMALL_ANY, LARGE_ODD), ids=_ids)
def test_maxpool3s2_emulated(emu_lib, kind, case):
    _run_maxpool3("cpu", kind, case)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", _cases(SMALL_ANY, LARGE_ODD), ids=_ids)
def test_maxpool3s2_gpu(hip_lib, kind, case):
    _run_maxpool3("cuda", kind, case)


# ---- FPN top-down add and its backward -------------------------------------------------------------------------------------------
def _run_upsample2(dev, kind, case, carry_sliced):
    (N, H, W, C), large = case
    if large:
        R.assert_two_uneven_trips(R.items_full(N, H, W, C), R.EW_CAP, C)
        R.assert_two_uneven_trips(R.items_pool2(N, H, W, C), R.EW_CAP, C)
    lat, top = _vals(kind, (N, H, W, C), 13, dev), _vals(kind, (N, H // 2, W // 2, C), 14, dev)
    out = _nan(lat.shape, dev)
    _call("omni_upsample2_add", lat, top, out, N, H, W, C)
    _same(out, R.upsample2_add(lat, top))           # one rounding of an exact float64 sum
    dout = _vals(kind, (N, H, W, C), 15, dev)
    dtop = _nan(top.shape, dev)
    _call("omni_upsample2_bwd", dout, dtop, N, H, W, C)
    t_abs = R.upsample2_bwd(dout, absolute=True)
    _close(dtop, R.upsample2_bwd(dout), kind, R.gamma(R.UPSAMPLE_BWD_CHAIN) * t_abs)
    carry, ldc = _carry(kind, top.shape, 16, dev, carry_sliced)
    dtop = _nan(top.shape, dev)
    _call("omni_upsample2_bwd_carry", dout, carry, ldc, dtop, N, H, W, C)
    _close(dtop, R.upsample2_bwd(dout) + carry.double(), kind,
           R.gamma(R.UPSAMPLE_BWD_CHAIN + R.CARRY_CHAIN) * (t_abs + carry.double().abs()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("carry_sliced", [False, True])
@pytest.mark.parametrize("case", _cases(SMALL_EVEN, LARGE_FPN), ids=_ids)
def test_upsample2_emulated(emu_lib, kind, case, carry_sliced):
    _run_upsample2("cpu", kind, case, carry_sliced)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("carry_sliced", [False, True])
@pytest.mark.parametrize("case", _cases(SMALL_EVEN, LARGE_FPN), ids=_ids)
def test_upsample2_gpu(hip_lib, kind, case, carry_sliced):
    _run_upsample2("cuda", kind, case, carry_sliced)


# ---- ReLU backward ---------------------------------------------------------------------------------------------------------------
RELU_LARGE = 4 * (R.EW_CAP + 777)


def _run_relu_bwd(dev, kind, n):
    if n == RELU_LARGE:
        R.assert_two_uneven_trips(n // 4, R.EW_CAP)
    dy, y = _vals(kind, (n,), 17, dev), _vals("randn", (n,), 18, dev)
    y[0::7] = 0.0           # the mask is y > 0: both zeros and every negative value block, +inf passes
    y[3::11] = -0.0
    y[5::13] = float("inf")
    y[6::17] = float("-inf")
    dz = _nan((n,), dev)
    _call("omni_relu_bwd", dy, y, dz, n)
    _same(dz, R.relu_bwd(dy, y))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [0, 4, 12, 1028, RELU_LARGE])
def test_relu_bwd_emulated(emu_lib, kind, n):
    _run_relu_bwd("cpu", kind, n)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [0, 4, 12, 1028, RELU_LARGE])
def test_relu_bwd_gpu(hip_lib, kind, n):
    _run_relu_bwd("cuda", kind, n)


# ---- image normalisation ---------------------------------------------------------------------------------------------------------
MEAN, STD = [103.530, 116.280, 123.675], [57.375, 57.120, 58.395]
# (N, H, W, PH, PW, image_hw rows or None, large)
PRE_SMALL_HW = [[9, 11], [5, 11], [9, 1], [0, 0], [20, 30]]      # full slot, shorter, width 1, all padding, larger than the slot (clamped)
PRE_CASES = [
    (5, 9, 11, 12, 16, PRE_SMALL_HW, False),
    (2, 2, 3, 2, 3, [[2, 3], [1, 2]], False),                    # no divisibility padding
    (1, 1, 1, 4, 4, [[1, 1]], False),
    (0, 4, 4, 4, 4, [], False),
]
PRE_LARGE = (3, 401, 437, 416, 448, [[401, 437], [123, 437], [500, 1]], True)      # divisibility 32: 559 104 pixels


def _run_preprocess(dev, case):
    N, H, W, PH, PW, hw_rows, large = case
    if large:
        R.assert_two_uneven_trips(N * PH * PW, R.EW_CAP)
    g = torch.Generator().manual_seed(19)
    imgs = [torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8).to(dev) for _ in range(N)]
    stacked = torch.stack(imgs) if N else torch.zeros((0, 3, H, W), dtype=torch.uint8, device=dev)
    hw = torch.tensor(hw_rows, dtype=torch.int32).reshape(N, 2).to(dev)
    norm = [float(v) for v in MEAN + STD]
    ptrs = (ctypes.c_void_p * max(N, 1))(*[im.data_ptr() for im in imgs])
    host_ptrs = ctypes.cast(ptrs, ctypes.c_void_p)
    for masked in (False, True):
        ref = R.preprocess(stacked, MEAN, STD, PH, PW, hw if masked else None)
        out = _nan((N, PH, PW, 4), dev)
        if masked:
            _call("omni_preprocess_masked", stacked, hw, out, N, H, W, PH, PW, *norm)
        else:
            _call("omni_preprocess", stacked, out, N, H, W, PH, PW, *norm)
        assert torch.equal(out, ref)
        out = _nan((N, PH, PW, 4), dev)
        _call("omni_preprocess_multi", host_ptrs, hw if masked else None, out, N, H, W, PH, PW, *norm)
        assert torch.equal(out, ref)
        # what the reference itself must be: fp32 (img - mean) / std inside the valid region, exact zeros everywhere else
        if N:
            plain = (stacked.float() - torch.tensor(MEAN, device=dev).view(1, 3, 1, 1)) / torch.tensor(STD, device=dev).view(1, 3, 1, 1)
            for n in range(N):
                vh, vw = (min(H, hw_rows[n][0]), min(W, hw_rows[n][1])) if masked else (H, W)
                assert torch.equal(ref[n, :vh, :vw, :3], plain[n, :, :vh, :vw].permute(1, 2, 0))
                assert ref[n, vh:].abs().sum() == 0 and ref[n, :, vw:].abs().sum() == 0 and ref[n, ..., 3].abs().sum() == 0


@pytest.mark.parametrize("case", PRE_CASES + [PRE_LARGE], ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}")
def test_preprocess_emulated(emu_lib, case):
    _run_preprocess("cpu", case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PRE_CASES + [PRE_LARGE], ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}")
def test_preprocess_gpu(hip_lib, case):
    _run_preprocess("cuda", case)


def _run_preprocess_list(dev):
    """bnpool.preprocess_list == bnpool.preprocess(torch.stack(...)); 64 images are taken, 65 and mixed shapes are declined"""
    from omni3d_amd.kernels import bnpool
    g = torch.Generator().manual_seed(20)
    imgs = [torch.randint(0, 256, (3, 5, 7), generator=g, dtype=torch.uint8).to(dev) for _ in range(65)]
    hw = torch.tensor([[5 - n % 3, 7 - n % 4] for n in range(64)], dtype=torch.int32).to(dev)
    for n, image_hw in ((3, None), (64, None), (64, hw)):
        got = bnpool.preprocess_list(imgs[:n], MEAN, STD, 4, image_hw=image_hw)
        want = bnpool.preprocess(torch.stack(imgs[:n]), MEAN, STD, 4, image_hw=image_hw)
        assert got.shape == (n, 4, 8, 8) and torch.equal(got, want)
        assert torch.equal(got.permute(0, 2, 3, 1), R.preprocess(torch.stack(imgs[:n]), MEAN, STD, 8, 8, image_hw))
    assert bnpool.preprocess_list(imgs, MEAN, STD, 4) is None
    assert bnpool.preprocess_list(imgs[:2] + [imgs[2][:, :4]], MEAN, STD, 4) is None
    assert bnpool.preprocess_list([], MEAN, STD, 4) is None


def test_preprocess_list_emulated(emu_lib):
    _run_preprocess_list("cpu")


@pytest.mark.gpu
def test_preprocess_list_gpu(hip_lib):
    _run_preprocess_list("cuda")


# ---- bias gradient ---------------------------------------------------------------------------------------------------------------
# (P, C): the 512-row cap; two channel tiles (288 quads); 256 % 5 != 0 leaves idle threads; a mid size whose accumulate == 1 takes
# the atomic kernel on the GPU with its 4-deep load loop running
BIAS_CASES = [(300000, 8), (2100, 1152), (37, 20), (5000, 24), (1, 4)]


def _run_bias_grad(dev, kind, PC, accumulate):
    P, C = PC
    nblk = R.red_grid(P, C)
    if PC == (300000, 8):
        assert (P + 4 * 128 - 1) // (4 * 128) > 512 and nblk == 512
    if PC == (2100, 1152):
        assert C // 4 > 256 and nblk == 512
    if PC == (37, 20):
        assert 256 % (C // 4) != 0
    atomic = dev == "cuda" and accumulate == 1 and nblk <= 64
    if PC in ((37, 20), (5000, 24)):
        assert nblk <= 64                       # the small-tensor atomic branch on the GPU
    dy = _vals(kind, (P, C), 21, dev)
    db0 = _vals(kind, (C,), 22, dev)
    db = db0.clone() if accumulate else _nan((C,), dev)
    ws = torch.full((2 * C * 258,), NAN, dtype=torch.float64, device=dev)
    _call("omni_bias_grad", dy, P, C, db, ws, accumulate)
    ref, t_abs = R.bias_grad(dy), R.bias_grad(dy, absolute=True)
    if accumulate:
        ref, t_abs = ref + db0.double(), t_abs + db0.double().abs()
    L32, L64 = R.bias_grad_chain(P, C, accumulate, atomic)
    _close(db, ref, kind, (R.gamma(L32) + L64 * R.U64) * t_abs)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("accumulate", [0, 1, 3])
@pytest.mark.parametrize("PC", BIAS_CASES, ids=lambda pc: f"{pc[0]}x{pc[1]}")
def test_bias_grad_emulated(emu_lib, kind, PC, accumulate):
    _run_bias_grad("cpu", kind, PC, accumulate)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("accumulate", [0, 1, 3])
@pytest.mark.parametrize("PC", BIAS_CASES, ids=lambda pc: f"{pc[0]}x{pc[1]}")
def test_bias_grad_gpu(hip_lib, kind, PC, accumulate):
    _run_bias_grad("cuda", kind, PC, accumulate)


# ---- depthwise convolution -------------------------------------------------------------------------------------------------------
# ((N, H, W, C), R, stride, pad, large)
DW_SMALL = [((1, 2, 2, 4), 3, 1, 1, False), ((2, 2, 3, 8), 3, 2, 1, False), ((1, 1, 1, 4), 3, 1, 1, False), ((1, 3, 3, 4), 3, 1, 0, False),
            ((2, 5, 7, 12), 5, 1, 2, False), ((2, 6, 5, 8), 5, 2, 2, False), ((1, 9, 8, 4), 5, 2, 0, False), ((2, 7, 6, 8), 3, 2, 2, False),
            ((1, 40, 30, 260), 3, 1, 1, False),     # 65 quads: two channel blocks and 4 slices in the weight gradient
            ((0, 4, 4, 4), 3, 1, 1, False)]
DW_LARGE = [((2, 211, 211, 96), 3, 1, 1, True), ((2, 211, 211, 96), 5, 2, 2, True)]


def _run_dwconv(dev, kind, case):
    (N, H, W, C), Rk, stride, pad, large = case
    OH, OW = R.dw_out(H, W, Rk, stride, pad)
    if large:
        R.assert_two_uneven_trips(R.items_full(N, H, W, C), R.DW_CAP, C)                          # dgrad
        if stride == 1:
            R.assert_two_uneven_trips(R.items_dw_fwd(N, H, W, C, Rk, stride, pad), R.DW_CAP, C)   # forward
            slices = R.dw_wgrad_slices(N, H, W, C, Rk, stride, pad)
            assert slices > 64 and (N * OH * OW) % (4 * slices) != 0                              # many atomics per tap, ragged slices
    x, w, dy = _vals(kind, (N, H, W, C), 23, dev), _vals(kind, (Rk, Rk, C), 24, dev), _vals(kind, (N, OH, OW, C), 25, dev)
    y = _nan(dy.shape, dev)
    _call("omni_dwconv_fwd", x, w, y, N, H, W, C, Rk, stride, pad)
    _close(y, R.dwconv_fwd(x, w, stride, pad), kind, R.gamma(R.dw_fwd_chain(Rk)) * R.dwconv_fwd(x, w, stride, pad, absolute=True))
    dx = _nan(x.shape, dev)
    _call("omni_dwconv_dgrad", dy, w, dx, N, H, W, C, Rk, stride, pad)
    _close(dx, R.dwconv_dgrad(dy, w, H, W, stride, pad), kind,
           R.gamma(R.dw_dgrad_chain(Rk, stride)) * R.dwconv_dgrad(dy, w, H, W, stride, pad, absolute=True))
    dw = _nan(w.shape, dev)
    _call("omni_dwconv_wgrad", x, dy, dw, N, H, W, C, Rk, stride, pad)
    _close(dw, R.dwconv_wgrad(x, dy, Rk, stride, pad), kind,
           R.gamma(R.dw_wgrad_chain(N, H, W, C, Rk, stride, pad)) * R.dwconv_wgrad(x, dy, Rk, stride, pad, absolute=True))


def _dw_id(c):
    return "x".join(str(v) for v in c[0]) + f"-R{c[1]}s{c[2]}p{c[3]}"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", DW_SMALL + DW_LARGE, ids=_dw_id)
def test_dwconv_emulated(emu_lib, kind, case):
    _run_dwconv("cpu", kind, case)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", DW_SMALL + DW_LARGE, ids=_dw_id)
def test_dwconv_gpu(hip_lib, kind, case):
    _run_dwconv("cuda", kind, case)


# ---- argument contracts ----------------------------------------------------------------------------------------------------------
def _run_contracts(dev):
    z = torch.zeros(4096, device=dev)
    u8 = torch.zeros(4096, dtype=torch.uint8, device=dev)
    i32 = torch.zeros(16, dtype=torch.int32, device=dev)
    # a carry with odd H or W in the 2x2 max-pool backward
    _raises("omni_maxpool2_bwd_carry", z, z, 4, z, 4, z, 1, 3, 4, 4)
    _raises("omni_maxpool2_bwd_carry", z, z, 4, z, 4, z, 1, 4, 3, 4)
    # carry / dy pitch below C or no multiple of 4
    _raises("omni_maxpool2_bwd_carry", z, z, 8, z, 4, z, 1, 4, 4, 8)
    _raises("omni_maxpool2_bwd_carry", z, z, 6, None, 0, z, 1, 4, 4, 4)
    _raises("omni_subsample2_bwd_carry", z, None, 4, z, 1, 4, 4, 4)
    # odd extents in the FPN top-down kernels
    for H, W in ((3, 4), (4, 3)):
        _raises("omni_upsample2_add", z, z, z, 1, H, W, 4)
        _raises("omni_upsample2_bwd_carry", z, z, 4, z, 1, H, W, 4)
        _raises("omni_upsample2_bwd", z, z, 1, H, W, 4)
    # C % 4 != 0
    for name in ("omni_maxpool2_fwd", "omni_avgpool2_fwd", "omni_avgpool2_bwd", "omni_subsample2_fwd", "omni_subsample2_bwd", "omni_maxpool3s2_fwd"):
        _raises(name, z, z, 1, 4, 4, 6)
    for name in ("omni_maxpool2_bwd", "omni_maxpool3s2_bwd", "omni_upsample2_add"):
        _raises(name, z, z, z, 1, 4, 4, 6)
    _raises("omni_upsample2_bwd", z, z, 1, 4, 4, 6)
    _raises("omni_subsample2_bwd_carry", z, z, 8, z, 1, 4, 4, 6)
    _raises("omni_relu_bwd", z, z, z, 6)
    _raises("omni_bias_grad", z, 4, 6, z, z.double(), 0)
    # the 2x2 pools need a whole window
    _raises("omni_maxpool2_fwd", z, z, 1, 1, 4, 4)
    _raises("omni_avgpool2_fwd", z, z, 1, 4, 1, 4)
    # depthwise: R in {3, 5}, stride in {1, 2}, pad < R, C % 4 == 0
    for Rk, stride, pad, C in ((4, 1, 1, 4), (7, 1, 3, 4), (3, 3, 1, 4), (3, 0, 1, 4), (3, 1, 3, 4), (5, 1, 5, 4), (3, 1, 1, 6)):
        _raises("omni_dwconv_fwd", z, z, z, 1, 6, 6, C, Rk, stride, pad)
        _raises("omni_dwconv_dgrad", z, z, z, 1, 6, 6, C, Rk, stride, pad)
        _raises("omni_dwconv_wgrad", z, z, z, 1, 6, 6, C, Rk, stride, pad)
    # preprocess: the padded extent is at least the slot
    norm = [float(v) for v in MEAN + STD]
    _raises("omni_preprocess", u8, z, 1, 8, 8, 7, 8, *norm)
    _raises("omni_preprocess", u8, z, 1, 8, 8, 8, 7, *norm)
    _raises("omni_preprocess_masked", u8, i32, z, 1, 8, 8, 7, 8, *norm)
    ptrs = (ctypes.c_void_p * 65)(*([u8.data_ptr()] * 65))
    _raises("omni_preprocess_multi", ctypes.cast(ptrs, ctypes.c_void_p), None, z, 1, 8, 8, 7, 8, *norm)
    _raises("omni_preprocess_multi", ctypes.cast(ptrs, ctypes.c_void_p), None, z, 65, 2, 2, 2, 2, *norm)


def test_argument_contracts_emulated(emu_lib):
    _run_contracts("cpu")


@pytest.mark.gpu
def test_argument_contracts_gpu(hip_lib):
    _run_contracts("cuda")


# ---- the Python wrappers of omni3d_amd/kernels/bnpool.py, once per entry point -------------------------------------------------------
def _run_wrappers(dev):
    from omni3d_amd.kernels import bnpool

    def cl(t):      # NHWC values as the logical NCHW channels_last tensor the wrappers take
        return t.permute(0, 3, 1, 2)

    def nhwc(t):
        return t.permute(0, 2, 3, 1)
    N, H, W, C = 2, 6, 10, 12
    x = _vals("int", (N, H, W, C), 30, dev)
    dy2 = _vals("int", (N, H // 2, W // 2, C), 31, dev)
    carry, carry2 = _vals("int", (N, H, W, C), 32, dev), _vals("int", (N, H // 2, W // 2, C), 33, dev)
    _same(nhwc(bnpool.maxpool2_fwd(cl(x))), R.maxpool2_fwd(x))
    _same(nhwc(bnpool.maxpool2_bwd(cl(x), cl(dy2))), R.maxpool2_bwd(x, dy2))
    _same(nhwc(bnpool.maxpool2_bwd(cl(x), cl(_in_slice(dy2)[0]), carry=cl(_in_slice(carry)[0]))), R.maxpool2_bwd(x, dy2) + carry.double())
    _same(nhwc(bnpool.avgpool2_fwd(cl(x))), R.avgpool2_fwd(x))
    _same(nhwc(bnpool.avgpool2_bwd(cl(dy2), (H + 1, W + 1))), R.avgpool2_bwd(dy2, H + 1, W + 1))
    xo = _vals("int", (N, 5, 7, C), 34, dev)
    dyo = _vals("int", (N, 3, 4, C), 35, dev)
    co = _vals("int", (N, 5, 7, C), 36, dev)
    _same(nhwc(bnpool.subsample2_fwd(cl(xo))), R.subsample2_fwd(xo))
    _same(nhwc(bnpool.subsample2_bwd(cl(dyo), (5, 7))), R.subsample2_bwd(dyo, 5, 7))
    _same(nhwc(bnpool.subsample2_bwd(cl(dyo), (5, 7), carry=cl(_in_slice(co)[0]))), R.subsample2_bwd(dyo, 5, 7) + co.double())
    _same(nhwc(bnpool.maxpool3s2_fwd(cl(xo))), R.maxpool3s2_fwd(xo))
    _same(nhwc(bnpool.maxpool3s2_bwd(cl(xo), cl(dyo))), R.maxpool3s2_bwd(xo, dyo))
    _same(nhwc(bnpool.upsample2_add(cl(x), cl(dy2))), R.upsample2_add(x, dy2))
    _same(nhwc(bnpool.upsample2_bwd(cl(x))), R.upsample2_bwd(x))
    _same(nhwc(bnpool.upsample2_bwd(cl(x), carry=cl(_in_slice(carry2)[0]))), R.upsample2_bwd(x) + carry2.double())
    y = _vals("randn", (N, H, W, C), 37, dev)
    _same(bnpool.relu_bwd(x, y), R.relu_bwd(x, y))
    d2 = x.reshape(-1, C)
    _same(bnpool.bias_grad(d2), R.bias_grad(d2))
    acc = carry[0, 0, 0].clone()
    assert bnpool.bias_grad(d2, accum_into=acc) is None
    _same(acc, R.bias_grad(d2) + carry[0, 0, 0].double())
    g = torch.Generator().manual_seed(38)
    imgs = torch.randint(0, 256, (3, 3, 9, 11), generator=g, dtype=torch.uint8).to(dev)
    hw = torch.tensor([[9, 11], [4, 11], [9, 1]], dtype=torch.int32).to(dev)
    for image_hw in (None, hw):
        got = bnpool.preprocess(imgs, MEAN, STD, 8, image_hw=image_hw)
        assert got.shape == (3, 4, 16, 16) and torch.equal(nhwc(got), R.preprocess(imgs, MEAN, STD, 16, 16, image_hw))


def test_wrappers_emulated(emu_lib):
    _run_wrappers("cpu")


@pytest.mark.gpu
def test_wrappers_gpu(hip_lib):
    _run_wrappers("cuda")
