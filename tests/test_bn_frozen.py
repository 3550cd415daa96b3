"""Frozen BatchNorm with gradients (freeze_bn / MODEL.USE_BN False, tools/train_net.py:150-151 of the reference): an eval-mode
BatchNorm2d inside a training pass normalises with its running statistics, never writes them, and passes gradients to x, gamma, beta
and the residual (csrc/bn_pool.hip omni_bn_frozen_fwd / omni_bn_frozen_bwd, functional.batch_norm_frozen).  Judged against torch's
nn.BatchNorm2d in eval mode, in float64."""
import pytest
import torch
import torch.nn.functional as F

CL = torch.channels_last


def _cl(t):
    return t.contiguous(memory_format=CL)


def _params(C, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.5,
            torch.rand(C, generator=g) + 0.25)


def _run_kernel(dev, N, C, H, W, relu, with_res, pitched=False, carry=False, direct=False):
    import omni3d_amd.functional as HF
    from omni3d_amd.kernels import bnpool
    g = torch.Generator().manual_seed(7 * C + H)
    gamma, beta, rm, rv = _params(C, C + W)
    x = torch.randn(N, C, H, W, generator=g) * 1.5 + 0.3
    res = torch.randn(N, C, H, W, generator=g) if with_res else None
    dy = torch.randn(N, C, H, W, generator=g)
    dpool = torch.randn(N, C, H // 2, W // 2, generator=g) if carry else None
    eps = 1e-5

    # float64 yardstick: torch's eval-mode BatchNorm (+ residual, ReLU); the residual's second consumer is a 2x2 max-pool
    xd = x.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rd = res.double().requires_grad_(True) if with_res else None
    z = F.batch_norm(xd, rm.double(), rv.double(), gd, bd, False, 0.1, eps)
    if with_res:
        z = z + rd
    z = F.relu(z) if relu else z
    loss = (z * dy.double()).sum()
    if carry:
        loss = loss + (F.max_pool2d(rd, 2, 2) * dpool.double()).sum()
    loss.backward()

    # kernels
    rm_k, rv_k = rm.to(dev), rv.to(dev)
    rm0, rv0 = rm_k.clone(), rv_k.clone()
    xk = _cl(x).to(dev).requires_grad_(True)
    gk, bk = gamma.to(dev).requires_grad_(True), beta.to(dev).requires_grad_(True)
    prefill = None
    if direct:      # the flat optimizers' protocol: the backward ADDS into the parameters' bucket views and returns no gradient
        prefill = (torch.randn(C, generator=g).to(dev), torch.randn(C, generator=g).to(dev))
        gk.grad, bk.grad = prefill[0].clone(), prefill[1].clone()
        gk._omni_direct_grad = bk._omni_direct_grad = True
    r0 = _cl(res).to(dev).requires_grad_(True) if with_res else None
    r = None
    if with_res:
        r = r0 * 1.0
        if carry:
            HF.fanout(r)
    y = HF.batch_norm_frozen(xk, gk, bk, rm_k, rv_k, r, relu, eps)
    # the eval-mode output of layers.BatchNorm2d: the same arithmetic, bit for bit where the kernel's rsqrt is torch's (the host build;
    # on the GPU the device library's rsqrtf and torch's rsqrt differ in the last bit for some values)
    scale = gamma.to(dev) * torch.rsqrt(rv_k + eps)
    cached = bnpool.bn_apply(xk.detach(), torch.cat([scale, beta.to(dev) - rm_k * scale]).contiguous(),
                             r.detach() if with_res else None, relu)
    if dev == "cpu":
        assert torch.equal(y.detach(), cached)
    else:
        assert float((y.detach() - cached).abs().max()) <= 1e-6 * max(1.0, float(cached.abs().max()))
    dyk = _cl(dy).to(dev)
    if pitched:     # dy as a channel slice of a wider NHWC gradient (the DLA Root's concatenated gradient)
        wide = torch.randn(N, H, W, C + 8, generator=g).to(dev)
        wide[..., 4:4 + C] = dyk.permute(0, 2, 3, 1)
        dyk = wide[..., 4:4 + C].permute(0, 3, 1, 2)
        assert not dyk.is_contiguous(memory_format=CL)
    outs, grads = [y], [dyk]
    if carry:       # made after the BatchNorm: the max-pool's backward runs first and leaves the carry in the slot
        outs.append(HF.max_pool2(r))
        grads.append(_cl(dpool).to(dev))
    torch.autograd.backward(outs, grads)
    assert torch.equal(rm_k, rm0) and torch.equal(rv_k, rv0)      # running statistics are never written

    def close(got, want, tol):
        got = got.detach().double().cpu()
        assert float((got - want).abs().max()) <= tol * max(1.0, float(want.abs().max())), float((got - want).abs().max())

    close(y, z.detach(), 2e-6)
    close(xk.grad, xd.grad, 2e-6)
    gg, gb = (gk.grad - prefill[0], bk.grad - prefill[1]) if direct else (gk.grad, bk.grad)
    close(gg, gd.grad, 2e-5)
    close(gb, bd.grad, 2e-5)
    if with_res:
        close(r0.grad, rd.grad, 2e-6)
    return xk, gk, bk, rm_k, rv_k, r, dyk


KERNEL_CASES = [
    (2, 16, 6, 10, True, False, False, False, False),
    (1, 64, 8, 8, False, True, False, False, False),
    (2, 128, 4, 6, True, True, False, True, False),       # residual with gradient fan-in (carry)
    (2, 32, 5, 7, True, False, True, False, False),       # pitched dy
    (1, 256, 3, 5, False, False, False, False, True),     # direct accumulation into pre-filled gradient buffers
    (2, 512, 2, 4, True, True, True, True, True),         # everything at once
    (1, 60, 7, 3, True, False, False, False, False),      # C % 16 != 0: a partial channel group
]


@pytest.mark.parametrize("cfg", KERNEL_CASES)
def test_frozen_bn_kernels_emulated(emu_lib, cfg):
    _run_kernel("cpu", *cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", KERNEL_CASES + [(4, 16, 128, 128, True, False, False, False, True), (4, 64, 64, 64, True, True, False, True, True)])
def test_frozen_bn_kernels_gpu(hip_lib, cfg):
    _run_kernel("cuda", *cfg)


def _run_determinism_and_masks(dev):
    """two runs give the same bits; the ReLU mask recomputed from x equals the one read from y"""
    from omni3d_amd.kernels import bnpool
    g = torch.Generator().manual_seed(5)
    N, C, H, W = 2, 48, 33, 17
    gamma, beta, rm, rv = [t.to(dev) for t in _params(C, 3)]
    x = _cl(torch.randn(N, C, H, W, generator=g)).to(dev)
    dy = _cl(torch.randn(N, C, H, W, generator=g)).to(dev)
    y = bnpool.bn_frozen_fwd(x, gamma, beta, rm, rv, None, True)
    assert torch.equal(y, bnpool.bn_frozen_fwd(x, gamma, beta, rm, rv, None, True))
    a = bnpool.bn_frozen_bwd(x, dy, y, gamma, beta, rm, rv, relu=True)
    b = bnpool.bn_frozen_bwd(x, dy, y, gamma, beta, rm, rv, relu=True)
    c = bnpool.bn_frozen_bwd(x, dy, None, gamma, beta, rm, rv, relu=True, remask=True)
    for u, v, w in zip(a, b, c):
        if u is not None:
            assert torch.equal(u, v) and torch.equal(u, w)
    dx, _, dg, db = bnpool.bn_frozen_bwd(x, dy, y, gamma, beta, rm, rv, relu=True, param_grads=False)
    assert torch.equal(dx, a[0]) and dg is None and db is None


def test_frozen_bn_deterministic_emulated(emu_lib):
    _run_determinism_and_masks("cpu")


@pytest.mark.gpu
def test_frozen_bn_deterministic_gpu(hip_lib):
    _run_determinism_and_masks("cuda")


def _run_module(dev):
    """layers.BatchNorm2d in eval mode: with gradients wanted it takes the frozen path, whose output equals the inference path's; the
    backbone below it gets gradients; running statistics and num_batches_tracked stay as they were"""
    from omni3d_amd.cubercnn.modeling.layers import BatchNorm2d, Conv2d, training_pass
    from omni3d_amd.cubercnn.solver.build import freeze_bn
    torch.manual_seed(0)
    conv, bn = Conv2d(16, 32, 3, padding=1, bias=False).to(dev), BatchNorm2d(32).to(dev)
    x = _cl(torch.randn(2, 16, 12, 12)).to(dev)
    with torch.no_grad():       # non-trivial running statistics
        for _ in range(3):
            bn(conv(x * 2 + 1))
    net = torch.nn.ModuleList([conv, bn])
    net.train()
    freeze_bn(net)
    assert conv.training and not bn.training and not bn.track_running_stats
    state = {k: v.clone() for k, v in bn.state_dict().items()}
    res = _cl(torch.randn(2, 32, 12, 12)).to(dev)
    with torch.no_grad():
        want = bn(conv(x), residual=res, relu=True)
    # outside a training pass an eval-mode BatchNorm is an inference layer, with or without gradients enabled: today's bits
    assert torch.equal(bn(conv(x), residual=res, relu=True).detach(), want)
    with training_pass():
        y = bn(conv(x), residual=res, relu=True)
        # the convolution stops emitting batch statistics once it knows its BatchNorm is frozen
        assert conv.__dict__.get("_stats_reader") is bn
        assert getattr(conv(x), "_omni_bn_partials", None) is None
    assert y.grad_fn is not None and "Frozen" in type(y.grad_fn).__name__
    assert float((y.detach() - want).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max()))
    if dev == "cpu":
        assert torch.equal(y.detach(), want)
    (y * y).sum().backward()
    assert float(conv.weight.grad.abs().max()) > 0 and float(bn.weight.grad.abs().max()) > 0 and float(bn.bias.grad.abs().max()) > 0
    for k, v in bn.state_dict().items():
        assert torch.equal(v, state[k]), k
    # the same layer in training mode still has the conv emit its statistics
    bn.train()
    bn(conv(x))
    assert getattr(conv(x), "_omni_bn_partials", None) is not None


def test_frozen_bn_module_emulated(emu_lib):
    _run_module("cpu")


@pytest.mark.gpu
def test_frozen_bn_module_gpu(hip_lib):
    _run_module("cuda")


def _run_shufflenet(dev):
    """ShuffleNet's 58-channel layers go through `_bn` with channels padded to 60"""
    from omni3d_amd.cubercnn.modeling.backbone import shufflenet as S
    from omni3d_amd.cubercnn.modeling.layers import BatchNorm2d, training_pass
    g = torch.Generator().manual_seed(9)
    m = BatchNorm2d(58)
    gamma, beta, rm, rv = _params(58, 58)
    with torch.no_grad():
        m.weight.copy_(gamma), m.bias.copy_(beta), m.running_mean.copy_(rm), m.running_var.copy_(rv)
    m = m.to(dev).eval()
    x = torch.randn(2, 58, 9, 11, generator=g)
    dy = torch.randn(2, 58, 9, 11, generator=g)
    xd = x.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z = F.relu(F.batch_norm(xd, rm.double(), rv.double(), gd, bd, False, 0.1, m.eps))
    z.backward(dy.double())
    xk = _cl(x).to(dev).requires_grad_(True)
    with torch.no_grad():
        want = S._bn(xk, m, relu=True)
    with training_pass():
        y = S._bn(xk, m, relu=True)
    assert float((y.detach() - want).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max()))
    if dev == "cpu":
        assert torch.equal(y.detach(), want)
    y.backward(dy.to(dev))
    z = z.detach()
    assert float((y.detach().double().cpu() - z).abs().max()) <= 2e-6 * max(1.0, float(z.abs().max()))
    for got, ref in ((xk.grad, xd.grad), (m.weight.grad, gd.grad), (m.bias.grad, bd.grad)):
        assert float((got.double().cpu() - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))
    assert torch.equal(m.running_mean.cpu(), rm) and torch.equal(m.running_var.cpu(), rv)


def test_frozen_bn_shufflenet_emulated(emu_lib):
    _run_shufflenet("cpu")


@pytest.mark.gpu
def test_frozen_bn_shufflenet_gpu(hip_lib):
    _run_shufflenet("cuda")
