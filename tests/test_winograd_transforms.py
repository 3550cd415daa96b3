"""Every Winograd transform kernel and fused epilogue of csrc/winograd.hip against its own definition in float64
(tests/ref_winograd.py), one stage at a time, then the whole convolution against a float64 F.conv2d.

Bounds (a priori, not fitted -- a kernel outside them is a finding):
  transforms   |got - ref64| <= 16 * 2^-24 * T_abs (+ 2^-24 * (|ref| + |bias| + |carry|)), T_abs = the transform with |matrix| on |input|
  statistics   |sum of the rows - sum64 over what the kernel wrote| <= L * 2^-24 * sum |term| per channel, L = ref_winograd.stats_chain
  convolution  the bounds of tests/test_conv.py (2e-6 for F(2x2), 1e-5 for F(4x4), times conv(|x|, |w|); 5x for the weight gradient)

Worst observed |error| / bound (every check prints its own as `wino-ratio`; run with -s), emulated build / MI355X, the MI355X
column including the large grid-stride cases:
  input 0.15 / 0.19        dy, dy_both 0.17 / 0.24      dy_both against the separate kernels 0 / 0 (bit-identical)
  output 0.16 / 0.16       + bias (+ReLU) 0.17 / 0.23   + carry 0.18 / 0.23
  U 0.28 / 0.28            U' 0.27 / 0.27               weights_multi 0.29 / 0.28
  dweights 0.21 / 0.21     accum_into 0.26 / 0.26
  forward statistics       y 0.16 / 0.16    sum y 0.04 / 0.04        sum y^2 0.11 / 0.09     (natural grid and capped)
  backward statistics      dx 0.15 / 0.15   sum dz 0.01 / 0.01       sum dz xhat 0.02 / 0.02
  convolution F(2x2)       y, dgrad 0.03 / 0.03    wgrad 0.02 / 0.02      F(4x4): y 0.03 / 0.03, dgrad 0.02 / 0.02, wgrad 0.01 / 0.01
  functional.conv2d        chosen = f22_only 0.05 / 0.05     F(4x4) 0.07 / 0.06     direct 0.006 / 0.006
"""
import pytest
import torch
import torch.nn.functional as F

import ref_winograd as R

TILES = (2, 4)
CL = torch.channels_last


def _note(name, dev, ratio):
    print("wino-ratio %-40s %-4s %.4f" % (name, dev, ratio))
    return ratio


def _check(name, dev, got, ref, bound):
    assert tuple(got.shape) == tuple(ref.shape), (name, got.shape, ref.shape)
    ratio = _note(name, dev, R.worst_ratio(got, ref, bound))
    assert ratio <= 1.0, (name, dev, ratio)


def _gen(dev, numel, seed):
    """a seeded generator: on the CPU (the same inputs on both builds), except for the large GPU-only cases"""
    return torch.Generator(device=dev if numel > (1 << 22) else "cpu").manual_seed(seed)


def _acts(dev, N, H, W, C, seed):
    """logical (N,C,H,W) tensor in NHWC memory: randn + a per-channel offset in [-2, 2] (real inputs are post-ReLU, not centred)"""
    g = _gen(dev, N * H * W * C, seed)
    x = torch.randn(N, H, W, C, generator=g, device=g.device) + (torch.rand(C, generator=g, device=g.device) * 4 - 2)
    return x.to(dev).permute(0, 3, 1, 2)


def _points(dev, tile, T, K, seed, offset=2.0):
    """a Winograd-domain tensor (P,T,K): randn + a per-channel offset in [-offset, offset]"""
    g = _gen(dev, (tile + 2) ** 2 * T * K, seed)
    m = torch.randn((tile + 2) ** 2, T, K, generator=g, device=g.device)
    return (m + (torch.rand(K, generator=g, device=g.device) * 2 - 1) * offset).to(dev)


def _krsc(dev, K, C, seed, scale=0.2):
    """logical (K,C,3,3) filter in KRSC memory"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(K, 3, 3, C, generator=g) * scale).to(dev).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _act_shapes(tile):
    return [(1, tile, tile, 4),                 # one tile, every border padded
            (2, 3 * tile, 2 * tile, 8),         # H != W, tile indices wrap rows and images
            (3, tile, 5 * tile, 24),            # C/4 = 6 does not divide 256: a thread's channel group changes between iterations
            (1, 2 * tile, 2 * tile, 260)]


# the smallest maps whose N (H/tile) (W/tile) C/4 exceeds the 4096 x 256 threads of the capped grid (C/4 = 260, no power of two):
# the grid-stride loops run more than once
BIG = {2: (1, 128, 128, 1040), 4: (1, 256, 256, 1040)}


# ---- 1. activation-side transforms -------------------------------------------------------------------------------------------
def _run_input(dev, tile, shape, seed=11):
    from omni3d_amd.kernels import wino
    x = _acts(dev, *shape, seed=seed)
    V = wino.transform_input(x, tile)
    xv = _nhwc(x)
    _check("input %s" % (shape,), dev, V, R.input_transform(xv, tile), R.transform_bound(R.input_transform(xv, tile, True)))


def _run_dy(dev, tile, shape, seed=12):
    from omni3d_amd.kernels import wino
    dy = _acts(dev, *shape, seed=seed)
    dv = _nhwc(dy)
    ref_dM, ref_Vd = R.dy_transform(dv, tile), R.input_transform(dv, tile)
    b_dM, b_Vd = R.transform_bound(R.dy_transform(dv, tile, True)), R.transform_bound(R.input_transform(dv, tile, True))
    dM1 = wino.transform_dy(dy, tile)
    _check("dy %s" % (shape,), dev, dM1, ref_dM, b_dM)
    dM, Vd = wino.transform_dy_both(dy, tile)
    _check("dy_both dM %s" % (shape,), dev, dM, ref_dM, b_dM)
    _check("dy_both Vd %s" % (shape,), dev, Vd, ref_Vd, b_Vd)
    # ... and against the two separate kernels, within the same bound
    _check("dy_both dM vs dy %s" % (shape,), dev, dM, dM1.double(), b_dM)
    _check("dy_both Vd vs input %s" % (shape,), dev, Vd, wino.transform_input(dy, tile).double(), b_Vd)


def _run_output(dev, tile, shape, seed=13, modes=("plain", "bias", "bias_relu", "carry", "carry_slice")):
    from omni3d_amd.kernels import wino
    N, H, W, K = shape
    M = _points(dev, tile, N * (H // tile) * (W // tile), K, seed)
    g = torch.Generator().manual_seed(seed + 100)
    ref, t_abs = R.output_transform(M, (N, H, W)), R.output_transform(M, (N, H, W), True)
    for mode in modes:
        if mode == "plain":
            y = wino.transform_output(M, (N, H, W))
            want, bound = ref, R.transform_bound(t_abs)
        elif mode in ("bias", "bias_relu"):
            bias = torch.randn(K, generator=g).to(dev)
            y = wino.transform_output(M, (N, H, W), bias, relu=(mode == "bias_relu"))
            want = ref + bias.double()
            if mode == "bias_relu":
                want = want.clamp(min=0)
            bound = R.transform_bound(t_abs, want, bias)
        else:
            if mode == "carry":
                carry = (torch.randn(N, H, W, K, generator=g) * 3).to(dev).permute(0, 3, 1, 2)
            else:   # a channel slice of a wider NHWC tensor: pixel pitch K + 8, first channel 4 (16-byte aligned)
                wide = (torch.randn(N, H, W, K + 8, generator=g) * 3).to(dev)
                carry = wide[..., 4:4 + K].permute(0, 3, 1, 2)
                assert carry.stride(3) == K + 8 and carry.data_ptr() % 16 == 0
            y = wino.transform_output(M, (N, H, W), carry=carry)
            cv = _nhwc(carry).double()
            want = ref + cv
            bound = R.transform_bound(t_abs, want, cv)
        _check("output %s %s" % (mode, shape), dev, _nhwc(y), want, bound)


@pytest.mark.parametrize("tile", TILES)
def test_input_transform_emulated(emu_lib, tile):
    for shape in _act_shapes(tile):
        _run_input("cpu", tile, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", TILES)
def test_input_transform_gpu(hip_lib, tile):
    for shape in _act_shapes(tile):
        _run_input("cuda", tile, shape)


@pytest.mark.parametrize("tile", TILES)
def test_dy_transforms_emulated(emu_lib, tile):
    for shape in _act_shapes(tile):
        _run_dy("cpu", tile, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", TILES)
def test_dy_transforms_gpu(hip_lib, tile):
    for shape in _act_shapes(tile):
        _run_dy("cuda", tile, shape)


@pytest.mark.parametrize("tile", TILES)
def test_output_transform_emulated(emu_lib, tile):
    for shape in _act_shapes(tile):
        _run_output("cpu", tile, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", TILES)
def test_output_transform_gpu(hip_lib, tile):
    for shape in _act_shapes(tile):
        _run_output("cuda", tile, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", TILES)
def test_input_transform_grid_stride_gpu(hip_lib, tile):
    N, H, W, C = BIG[tile]
    assert N * (H // tile) * (W // tile) * (C // 4) > 4096 * 256
    _run_input("cuda", tile, BIG[tile])


@pytest.mark.gpu
@pytest.mark.parametrize("tile", TILES)
def test_dy_transforms_grid_stride_gpu(hip_lib, tile):
    _run_dy("cuda", tile, BIG[tile])


@pytest.mark.gpu
@pytest.mark.parametrize("tile", TILES)
def test_output_transform_grid_stride_gpu(hip_lib, tile):
    _run_output("cuda", tile, BIG[tile], modes=("bias_relu", "carry"))


# ---- 2. filter-side transforms -----------------------------------------------------------------------------------------------
KC = [(1, 1), (32, 32), (33, 31), (48, 40), (40, 72), (96, 64)]


def _check_weights(name, dev, w, tile, U, Uf, want_u, want_flip):
    assert (U is not None) == want_u and (Uf is not None) == want_flip
    if want_u:
        _check("U %s" % name, dev, U, R.weights_transform(w, tile), R.transform_bound(R.weights_transform(w, tile, absolute=True)))
    if want_flip:
        _check("U' %s" % name, dev, Uf, R.weights_transform(w, tile, flip=True),
               R.transform_bound(R.weights_transform(w, tile, flip=True, absolute=True)))


def _run_weights(dev, tile):
    from omni3d_amd.kernels import wino
    for i, (K, C) in enumerate(KC):
        w = _krsc(dev, K, C, seed=20 + i)
        for want_u, want_flip in ((True, False), (False, True), (True, True)):
            U, Uf = wino.transform_weights(w, want_u, want_flip, tile)
            _check_weights("%s tile %d %d%d" % ((K, C), tile, want_u, want_flip), dev, w, tile, U, Uf, want_u, want_flip)


def _run_weights_multi(dev):
    from omni3d_amd.kernels import wino
    items = []
    for i, (K, C) in enumerate(KC):
        for tile in TILES:
            for j, (want_u, want_flip) in enumerate(((True, False), (False, True), (True, True))):
                items.append((_krsc(dev, K, C, seed=40 + 7 * i + j + 3 * tile), want_u, want_flip, tile))
    items = items[1::2] + items[0::2]       # shapes, tile sizes and outputs mixed
    assert len(items) <= wino.WEIGHTS_MULTI_MAX
    outs = wino.transform_weights_multi(items)
    assert len(outs) == len(items)
    for (w, want_u, want_flip, tile), (U, Uf) in zip(items, outs):
        _check_weights("multi %s tile %d %d%d" % (tuple(w.shape[:2]), tile, want_u, want_flip), dev, w, tile, U, Uf, want_u, want_flip)


def _run_dweights(dev, tile):
    from omni3d_amd.kernels import wino
    for i, (K, C) in enumerate(KC):
        g = torch.Generator().manual_seed(60 + i)
        dU = torch.randn((tile + 2) ** 2, K, C, generator=g).to(dev)
        ref, t_abs = R.dweights_transform(dU), R.dweights_transform(dU, True)
        dw = wino.transform_dweights(dU)
        assert _nhwc(dw).is_contiguous()
        _check("dweights %s tile %d" % ((K, C), tile), dev, dw, ref, R.transform_bound(t_abs))
        # accum_into a non-zero view inside a larger buffer: the float64 sum, and nothing written around it
        base = torch.randn(K * 9 * C + 16, generator=g).to(dev)
        before = base.clone()
        view = base[8:8 + K * 9 * C].view(K, 3, 3, C).permute(0, 3, 1, 2)
        old = view.double().clone()
        assert wino.transform_dweights(dU, accum_into=view) is None
        _check("dweights accum %s tile %d" % ((K, C), tile), dev, view, ref + old, R.transform_bound(t_abs, ref + old, old))
        assert torch.equal(base[:8], before[:8]) and torch.equal(base[-8:], before[-8:])


@pytest.mark.parametrize("tile", TILES)
def test_weights_transform_emulated(emu_lib, tile):
    _run_weights("cpu", tile)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", TILES)
def test_weights_transform_gpu(hip_lib, tile):
    _run_weights("cuda", tile)


def test_weights_transform_multi_emulated(emu_lib):
    _run_weights_multi("cpu")


@pytest.mark.gpu
def test_weights_transform_multi_gpu(hip_lib):
    _run_weights_multi("cuda")


@pytest.mark.parametrize("tile", TILES)
def test_dweights_transform_emulated(emu_lib, tile):
    _run_dweights("cpu", tile)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", TILES)
def test_dweights_transform_gpu(hip_lib, tile):
    _run_dweights("cuda", tile)


# ---- 3. forward statistics ---------------------------------------------------------------------------------------------------
def _fwd_stats_shape(tile, K):
    """the smallest maps of 2 images whose natural grid (ref_winograd.natural_grid) has more than 3 workgroups, so that the caps at
    1 and 3 both bind"""
    return {8: (2, 16 * tile, 16 * tile), 64: (2, 4 * tile, 8 * tile), 128: (2, 4 * tile, 4 * tile), 256: (2, 4 * tile, 4 * tile)}[K]


def _check_sums(name, dev, parts, rows, K, terms0, terms1, L):
    """parts (rows, 2K) summed in float64 against the float64 sums of the per-element terms (., K) of both statistics"""
    assert parts is not None and tuple(parts.shape) == (rows, 2 * K), (name, None if parts is None else parts.shape, rows)
    got = parts.double().sum(0)
    for j, terms in enumerate((terms0, terms1)):
        terms = terms.reshape(-1, K)
        _check("%s sum%d" % (name, j), dev, got[j * K:(j + 1) * K], terms.sum(0), L * R.U32 * terms.abs().sum(0))


def _run_fwd_stats(dev, tile, K, monkeypatch):
    from omni3d_amd.kernels import conv, wino
    N, H, W = _fwd_stats_shape(tile, K)
    assert R.natural_grid(N, H, W, K, tile) > 3
    M = _points(dev, tile, N * (H // tile) * (W // tile), K, seed=70 + K, offset=0.5)
    ref, bound = R.output_transform(M, (N, H, W)), R.transform_bound(R.output_transform(M, (N, H, W), True))
    flat = ref.reshape(-1, K)
    assert bool((flat.mean(0).abs() <= flat.std(0)).all())        # centred enough for the fp32 sum of squares (as test_bn_*)
    for cap in (None, 1, 3):
        if cap is not None:
            monkeypatch.setattr(conv, "STATS_ROWS", cap)
        rows = R.stats_rows(N, H, W, K, tile, conv.STATS_ROWS)
        assert cap is None or rows == cap
        y, parts = wino.transform_output_stats(M, (N, H, W))
        name = "fwd stats tile %d K %d cap %s" % (tile, K, cap)
        _check(name + " y", dev, _nhwc(y), ref, bound)
        y64 = _nhwc(y).double()
        _check_sums(name, dev, parts, rows, K, y64, y64 * y64, R.stats_chain(N, H, W, K, tile, rows))


def _run_fwd_stats_refused(dev, tile, K):
    from omni3d_amd.kernels import wino
    N, H, W = 2, 4 * tile, 4 * tile
    assert 256 % (K // 4) != 0
    M = _points(dev, tile, N * (H // tile) * (W // tile), K, seed=80 + K, offset=0.5)
    y, parts = wino.transform_output_stats(M, (N, H, W))
    assert parts is None
    _check("fwd stats refused tile %d K %d" % (tile, K), dev, _nhwc(y), R.output_transform(M, (N, H, W)),
           R.transform_bound(R.output_transform(M, (N, H, W), True)))


@pytest.mark.parametrize("K", [8, 64, 128, 256])
@pytest.mark.parametrize("tile", TILES)
def test_forward_statistics_emulated(emu_lib, monkeypatch, tile, K):
    _run_fwd_stats("cpu", tile, K, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [8, 64, 128, 256])
@pytest.mark.parametrize("tile", TILES)
def test_forward_statistics_gpu(hip_lib, monkeypatch, tile, K):
    _run_fwd_stats("cuda", tile, K, monkeypatch)


@pytest.mark.parametrize("K", [24, 96])
@pytest.mark.parametrize("tile", TILES)
def test_forward_statistics_refused_emulated(emu_lib, tile, K):
    _run_fwd_stats_refused("cpu", tile, K)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [24, 96])
@pytest.mark.parametrize("tile", TILES)
def test_forward_statistics_refused_gpu(hip_lib, tile, K):
    _run_fwd_stats_refused("cuda", tile, K)


# ---- 4. backward statistics --------------------------------------------------------------------------------------------------
def _bn_inputs(dev, N, H, W, K, seed, relu):
    """bn_x (N,K,H,W) CL, mean_rstd (2K), scale_shift (2K) or None; with the ReLU no element has |bn_x * scale + shift| < 1e-4
    (offenders are nudged away from zero), so a fused multiply-add in the kernel cannot flip a mask bit"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, K, generator=g) * (torch.rand(K, generator=g) + 0.5) + torch.randn(K, generator=g)
    flat = x.reshape(-1, K)
    mean_rstd = torch.cat([flat.mean(0), 1.0 / (flat.var(0, unbiased=False) + 1e-5).sqrt()])
    scale_shift = None
    if relu:
        scale = (torch.rand(K, generator=g) + 0.5) * mean_rstd[K:] * torch.where(torch.rand(K, generator=g) < 0.25, -1.0, 1.0)
        shift = torch.randn(K, generator=g) * 0.5 - flat.mean(0) * scale
        z = x.double() * scale.double() + shift.double()
        near = z.abs() < 4e-4
        # move the offenders to |z| ~ 1e-3 on the side they are on
        x = torch.where(near, ((torch.where(z >= 0, 1e-3, -1e-3) - shift.double()) / scale.double()).float(), x)
        scale_shift = torch.cat([scale, shift])
        z = x.double() * scale.double() + shift.double()
        assert float(z.abs().min()) >= 1e-4
        assert 0.2 < float((z > 0).double().mean()) < 0.8
    return x.to(dev).permute(0, 3, 1, 2), mean_rstd.to(dev), (scale_shift.to(dev) if relu else None)


def _bwd_terms(dx, bn_x, mean_rstd, scale_shift, K):
    """dz and dz * xhat in float64 from the dx the kernel wrote"""
    x64, d64 = _nhwc(bn_x).double(), _nhwc(dx).double()
    if scale_shift is not None:
        d64 = d64 * ((x64 * scale_shift[:K].double() + scale_shift[K:].double()) > 0)
    return d64, d64 * ((x64 - mean_rstd[:K].double()) * mean_rstd[K:].double())


def _run_bwd_stats(dev, K, relu, monkeypatch):
    from omni3d_amd.kernels import conv, wino
    tile = 4
    N, H, W = {8: (2, 48, 48), 128: (2, 16, 16)}[K]        # natural grids of 3 and 4 workgroups
    assert R.natural_grid(N, H, W, K, tile) > 1
    M = _points(dev, tile, N * (H // tile) * (W // tile), K, seed=90 + K, offset=0.5)
    bn_x, mean_rstd, scale_shift = _bn_inputs(dev, N, H, W, K, 91 + K, relu)
    ref, bound = R.output_transform(M, (N, H, W)), R.transform_bound(R.output_transform(M, (N, H, W), True))
    for cap in (None, 1):
        if cap is not None:
            monkeypatch.setattr(conv, "STATS_ROWS", cap)
        rows = R.stats_rows(N, H, W, K, tile, conv.STATS_ROWS)
        assert cap is None or rows == cap
        dx, parts = wino.transform_output_bn_bwd(M, (N, H, W), bn_x, mean_rstd, scale_shift)
        name = "bwd stats K %d relu %d cap %s" % (K, relu, cap)
        _check(name + " dx", dev, _nhwc(dx), ref, bound)
        dz, dzx = _bwd_terms(dx, bn_x, mean_rstd, scale_shift, K)
        _check_sums(name, dev, parts, rows, K, dz, dzx, R.stats_chain(N, H, W, K, tile, rows))


def _run_bwd_stats_refused(dev, tile, K):
    from omni3d_amd.kernels import wino
    N, H, W = 2, 4 * tile, 4 * tile
    M = _points(dev, tile, N * (H // tile) * (W // tile), K, seed=95 + K, offset=0.5)
    for relu in (True, False):
        bn_x, mean_rstd, scale_shift = _bn_inputs(dev, N, H, W, K, 96 + K, relu)
        dx, parts = wino.transform_output_bn_bwd(M, (N, H, W), bn_x, mean_rstd, scale_shift)
        assert parts is None
        _check("bwd stats refused tile %d K %d relu %d" % (tile, K, relu), dev, _nhwc(dx), R.output_transform(M, (N, H, W)),
               R.transform_bound(R.output_transform(M, (N, H, W), True)))


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("K", [8, 128])
def test_backward_statistics_emulated(emu_lib, monkeypatch, K, relu):
    _run_bwd_stats("cpu", K, relu, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("K", [8, 128])
def test_backward_statistics_gpu(hip_lib, monkeypatch, K, relu):
    _run_bwd_stats("cuda", K, relu, monkeypatch)


@pytest.mark.parametrize("tile,K", [(2, 8), (2, 128), (4, 24)])
def test_backward_statistics_refused_emulated(emu_lib, tile, K):
    _run_bwd_stats_refused("cpu", tile, K)


@pytest.mark.gpu
@pytest.mark.parametrize("tile,K", [(2, 8), (2, 128), (4, 24)])
def test_backward_statistics_refused_gpu(hip_lib, tile, K):
    _run_bwd_stats_refused("cuda", tile, K)


# ---- 5. the whole convolution against float64 --------------------------------------------------------------------------------
def _conv_ref64(x, w, b, dy, relu):
    """float64 F.conv2d (+ReLU) with autograd -> (y, dz = dy masked by the ReLU, dx, dw, db), all float64 on the CPU"""
    xr, wr, br = [t.detach().cpu().double().requires_grad_(True) for t in (x, w, b)]
    y = F.conv2d(xr, wr, br, padding=1)
    if relu:
        y = F.relu(y)
    y.backward(dy.detach().cpu().double())
    dz = dy.detach().cpu().double() * (y.detach() > 0) if relu else dy.detach().cpu().double()
    return y.detach(), dz, xr.grad, wr.grad, br.grad


def _conv_inputs(dev, N, C, K, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = (F.relu(torch.randn(N, H, W, C, generator=g)) + 0.5).to(dev).permute(0, 3, 1, 2)
    w = _krsc(dev, K, C, seed + 1, scale=0.1)
    b = torch.randn(K, generator=g).to(dev)
    dy = torch.randn(N, H, W, K, generator=g).to(dev).permute(0, 3, 1, 2)
    return x, w, b, dy


def _err(a, b):
    return float((a.detach().cpu().double() - b).abs().max())


def _run_conv64(dev, tile, N, C, K, H, W, seed=3):
    """as _run_wino of tests/test_conv.py, same bounds, against float64"""
    from omni3d_amd.kernels import wino
    x, w, b, dy = _conv_inputs(dev, N, C, K, H, W, seed)
    y_ref, dz, dx_ref, dw_ref, _ = _conv_ref64(x, w, b, dy, relu=True)
    tol = 2e-6 if tile == 2 else 1e-5
    xa, wa = x.cpu().double().abs(), w.cpu().double().abs()
    s_y = float(F.conv2d(xa, wa, None, padding=1).max())
    s_dx = float(F.conv_transpose2d(dy.cpu().double().abs(), wa, padding=1).max())
    s_dw = max(1.0, float(dw_ref.abs().max()))
    name = "conv tile %d %s" % (tile, (N, C, K, H, W))
    y, V = wino.conv3x3_fwd(x, w, b, relu=True, tile=tile)
    assert V.shape[0] == (tile + 2) ** 2
    ratios = {"y": _err(y, y_ref) / (tol * s_y)}
    dzk = dz.float().contiguous(memory_format=CL).to(dev)
    ratios["dgrad"] = _err(wino.conv3x3_dgrad(dzk, w, tile=tile), dx_ref) / (tol * s_dx)
    ratios["wgrad"] = _err(wino.conv3x3_wgrad(V, dzk), dw_ref) / (5 * tol * s_dw)
    dx2, dw2 = wino.conv3x3_backward(V, dzk, w, None)
    ratios["backward dx"] = _err(dx2, dx_ref) / (tol * s_dx)
    ratios["backward dw"] = _err(dw2, dw_ref) / (5 * tol * s_dw)
    acc = torch.ones_like(w)
    assert wino.conv3x3_wgrad(V, dzk, accum_into=acc) is None
    ratios["wgrad accum"] = _err(acc, dw_ref + 1.0) / (5 * tol * s_dw)
    for k, r in ratios.items():
        _note("%s %s" % (name, k), dev, r)
    assert all(r <= 1.0 for r in ratios.values()), (name, ratios)


def _conv_shapes(tile):
    return [(2, 8, 12, 3 * tile, 2 * tile), (1, 24, 40, tile, tile), (3, 4, 4, 2 * tile, 5 * tile)]


@pytest.mark.parametrize("tile", TILES)
def test_convolution_float64_emulated(emu_lib, tile):
    for s in _conv_shapes(tile):
        _run_conv64("cpu", tile, *s)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", TILES)
def test_convolution_float64_gpu(hip_lib, tile):
    for s in _conv_shapes(tile):
        _run_conv64("cuda", tile, *s)


def _run_functional64(dev, monkeypatch):
    """functional.conv2d on (4,128,16,16): the path the dispatch chooses (F(2x2): 64 tiles of 4x4 are too few), the same inside
    wino.f22_only(), F(4x4) with its tile threshold lowered, and the direct implicit GEMM with the Winograd path switched off --
    forward and all three gradients against one float64 result"""
    import omni3d_amd.functional as HF
    from omni3d_amd.kernels import wino
    N, C, K, H, W = 4, 128, 128, 16, 16
    x, w, b, dy = _conv_inputs(dev, N, C, K, H, W, seed=17)
    y_ref, _, dx_ref, dw_ref, db_ref = _conv_ref64(x, w, b, dy, relu=False)
    xa, wa = x.cpu().double().abs(), w.cpu().double().abs()
    s_y = float(F.conv2d(xa, wa, None, padding=1).max())
    s_dx = float(F.conv_transpose2d(dy.cpu().double().abs(), wa, padding=1).max())
    s_dw = max(1.0, float(dw_ref.abs().max()))
    b_db = N * H * W * R.U32 * dy.cpu().double().abs().sum((0, 2, 3))        # a sum of N H W values, in whatever order
    seen = []
    real_in = wino.transform_input
    monkeypatch.setattr(wino, "transform_input", lambda t, tile=2: (seen.append(tile), real_in(t, tile))[1])

    def run(name, tol, want_tile):
        del seen[:]
        xs = [t.detach().clone().requires_grad_(True) for t in (x, w, b)]
        y = HF.conv2d(xs[0], xs[1], xs[2], 1, 1)
        y.backward(dy)
        assert (seen[0] if seen else None) == want_tile, (name, seen)
        ratios = {"y": _err(y, y_ref) / (tol * s_y), "dx": _err(xs[0].grad, dx_ref) / (tol * s_dx),
                  "dw": _err(xs[1].grad, dw_ref) / (5 * tol * s_dw), "db": R.worst_ratio(xs[2].grad.cpu(), db_ref, b_db)}
        for k, r in ratios.items():
            _note("functional %s %s" % (name, k), dev, r)
        assert all(r <= 1.0 for r in ratios.values()), (name, ratios)

    assert wino.eligible(x.shape, w.shape, 1, 1) and wino.tile_size(x.shape) == 2
    run("chosen", 2e-6, 2)
    with wino.f22_only():
        run("f22_only", 2e-6, 2)
    with monkeypatch.context() as m:
        m.setattr(wino, "_F43_MIN_TILES", 64)
        assert wino.tile_size(x.shape) == 4
        run("F(4x4)", 1e-5, 4)
    with monkeypatch.context() as m:
        m.setattr(wino, "eligible", lambda *a: False)
        run("direct", 2e-5, None)       # the bound of the direct kernels in tests/test_conv.py (_check)


def test_functional_conv_float64_emulated(emu_lib, monkeypatch):
    _run_functional64("cpu", monkeypatch)


@pytest.mark.gpu
def test_functional_conv_float64_gpu(hip_lib, monkeypatch):
    _run_functional64("cuda", monkeypatch)
