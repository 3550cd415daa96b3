"""Run-to-run determinism of the training step (missing #4).

The reference's PyTorch-CPU path gives identical results every time it runs.  Rounds 1-3 of the HIP path did not: split-K partial
tiles, the fc1 cut tiles, small bias gradients, the stem weight gradient and the ROIAlign scatter met in their outputs through fp32
atomics, so the rounding followed the order in which workgroups finished and two runs of the same step differed by 0.6-1.3 % (relative
L2) on bottom-up gradient tensors (profiles/r03_grad_run_to_run_spread.txt).  Round 4: ordered split reductions
(csrc/split_reduce.h), a fixed-order stem / bias finalize, an owner-computes ROIAlign backward.

  * emulated: the ordered forms compute the same numbers as the atomic forms (summation order aside) on split launches of every
    kernel family, and hand the workspace counters back zeroed;
  * GPU: two executions of the full-size training step (BASELINE configs[1]: 4 x 512 x 512, default config) give BIT-IDENTICAL
    losses and gradients for every parameter -- eager launches and staged hipGraph replays."""
import ctypes
import os

import pytest
import torch

from conftest import ROOT


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _both(fn):
    from omni3d_amd.kernels import detmode
    prev = detmode.set_enabled(True)
    try:
        a = fn()
        detmode.set_enabled(False)
        b = fn()
    finally:
        detmode.set_enabled(prev)
    return a, b


def _counters_clean():
    from omni3d_amd.kernels import detmode
    return all(int(c.abs().sum()) == 0 for c in detmode._counters.values())


def _run_ordered_equals_atomic(dev):
    from omni3d_amd.kernels import conv, gemm, wino, bnpool
    g = torch.Generator().manual_seed(4)
    # forward / data gradient / weight gradient with explicit reduction splits (ragged tiles, bias + ReLU on the split forward)
    x = _cl(torch.randn(2, 64, 10, 12, generator=g)).to(dev)
    w = _cl(torch.randn(72, 64, 3, 3, generator=g) * 0.1).to(dev)
    b = torch.randn(72, generator=g).to(dev)
    for splits in (1, 3, 5):
        ya, yb = _both(lambda: conv.conv2d_fwd(x, w, b, 1, 1, relu=True, tile=2, splits=splits))
        assert (ya - yb).abs().max() <= 2e-5 * float(yb.abs().max())
        dy = _cl(torch.randn(2, 72, 10, 12, generator=g)).to(dev)
        da, db = _both(lambda: conv.conv2d_dgrad(dy, w, (10, 12), 1, 1, tile=2, splits=splits))
        assert (da - db).abs().max() <= 2e-5 * float(db.abs().max())
        carry = _cl(torch.randn(2, 64, 10, 12, generator=g)).to(dev)
        ca, cb = _both(lambda: conv.conv2d_dgrad(dy, w, (10, 12), 1, 1, tile=2, splits=splits, accum_into=carry.clone()))
        assert (ca - cb).abs().max() <= 2e-5 * float(cb.abs().max())
    # strided data gradient: parity classes with empty splits
    ws2 = _cl(torch.randn(32, 64, 1, 1, generator=g)).to(dev)
    dy2 = _cl(torch.randn(2, 32, 5, 6, generator=g)).to(dev)
    sa, sb = _both(lambda: conv.conv2d_dgrad(dy2, ws2, (10, 12), 2, 0, tile=2, splits=2))
    assert (sa - sb).abs().max() <= 2e-5 * max(float(sb.abs().max()), 1e-6)
    dy = _cl(torch.randn(2, 72, 10, 12, generator=g)).to(dev)
    wa, wb = _both(lambda: conv.conv2d_wgrad(x, dy, (3, 3), 1, 1))                  # the launcher splits over pixels by itself
    assert (wa - wb).abs().max() <= 2e-5 * float(wb.abs().max())
    acc0 = _cl(torch.randn(72, 64, 3, 3, generator=g)).to(dev)

    def into_bucket():
        t = acc0.clone(memory_format=torch.channels_last)
        conv.conv2d_wgrad(x, dy, (3, 3), 1, 1, accum_into=t)
        return t
    aa, ab = _both(into_bucket)
    assert (aa - ab).abs().max() <= 2e-5 * float(ab.abs().max())
    # Winograd-domain weight gradient (row splits of gemm_tn_pf), the engine's split / balanced forms
    V, dM = torch.randn(16, 600, 64, generator=g).to(dev), torch.randn(16, 600, 64, generator=g).to(dev)
    ua, ub = _both(lambda: wino.gemm_batched_wgrad(V, dM))
    assert (ua - ub).abs().max() <= 2e-5 * float(ub.abs().max())
    A, B = torch.randn(300, 512, generator=g).to(dev), torch.randn(200, 512, generator=g).to(dev)
    bias = torch.randn(200, generator=g).to(dev)
    ea, eb = _both(lambda: gemm.gemm(A, B, gemm.NT, bias=bias, tile=2, splits=4))
    assert (ea - eb).abs().max() <= 2e-5 * float(eb.abs().max())
    er = gemm.gemm(A, B, gemm.NT, bias=bias, relu=True, tile=2, splits=4)            # ReLU on cut tiles: ordered form only
    assert (er - eb.clamp(min=0)).abs().max() <= 2e-5 * float(eb.abs().max())
    At, Bt = torch.randn(512, 300, generator=g).to(dev), torch.randn(512, 200, generator=g).to(dev)
    base = torch.randn(300, 200, generator=g).to(dev)
    ta, tb = _both(lambda: gemm.gemm(At, Bt, gemm.TN, out=base.clone(), accumulate=True, tile=2, splits=gemm.BALANCED, workgroups=8))
    assert (ta - tb).abs().max() <= 2e-5 * float(tb.abs().max())
    na, nb = _both(lambda: gemm.gemm(A, B, gemm.NT, tile=2, splits=gemm.BALANCED, workgroups=8))
    assert (na - nb).abs().max() <= 2e-5 * float(nb.abs().max())
    # stem weight gradient, bias gradient
    xs = _cl(torch.randn(1, 16, 9, 66, generator=g)).to(dev)
    dys = _cl(torch.randn(1, 16, 9, 66, generator=g)).to(dev)
    qa, qb = _both(lambda: conv.stem_conv_wgrad(xs, dys, 3))
    assert (qa - qb).abs().max() <= 2e-5 * float(qb.abs().max())
    d2 = torch.randn(700, 64, generator=g).to(dev)
    start = torch.randn(64, generator=g).to(dev)

    def bias_into():
        t = start.clone()
        bnpool.bias_grad(d2, accum_into=t)
        return t
    ba, bb = _both(bias_into)
    assert (ba - bb).abs().max() <= 2e-5 * float(bb.abs().max())
    assert _counters_clean()


def test_ordered_reductions_equal_atomic_ones_emulated(emu_lib):
    _run_ordered_equals_atomic("cpu")


@pytest.mark.gpu
def test_ordered_reductions_equal_atomic_ones_gpu(hip_lib):
    _run_ordered_equals_atomic("cuda")


class _PlanRecorder:
    """stand-in for the loaded library: records every call and answers a plan call (plan address set) with `report`"""

    def __init__(self, report):
        self.report, self.calls = report, []

    def call(self, name, *args):
        self.calls.append((name, args))
        if args[-2] is not None:
            plan = (ctypes.c_longlong * 4).from_address(args[-2])
            plan[0], plan[1], plan[2], plan[3] = self.report


def test_plan_launch_protocol():
    """detmode.plan_launch is the one implementation of the `plan` protocol of include/omni3d_hip.h: exactly two calls of the named entry --
    the plan call (plan address set, workspace / counters / launch-only arguments null) and the launch (plan null, the workspace and the
    counters the reported plan asks for) -- with the same leading arguments, the plan's answer in place of the request; a plan that
    reports no split allocates nothing when the domain's counter block exists"""
    from torch.utils._python_dispatch import TorchDispatchMode
    from omni3d_amd.kernels import detmode

    class Ops(TorchDispatchMode):
        seen = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.seen.append(func.__name__)
            return func(*args, **(kwargs or {}))

    like = torch.zeros(1)
    head = tuple(range(101, 117))       # omni_conv2d_fwd_det: 16 leading arguments up to `relu`
    with detmode.domain("plan-launch-test"):
        try:
            # split tail, request fed back (tile, splits), launch-only arguments (statistics buffer, rows, block-count cell)
            L = _PlanRecorder((2, 3, 5, 640))
            detmode.plan_launch(L, "omni_conv2d_fwd_det", like, head, ask=(0, 9), late=(7001, 64, 7002))
            block = detmode._counters[detmode._key(like)]
            assert [n for n, _ in L.calls] == ["omni_conv2d_fwd_det"] * 2
            (_, a), (_, b) = L.calls
            assert a[:16] == head and b[:16] == head
            assert a[16:18] == (0, 9) and a[18:21] == (None, 0, None) and a[21:25] == (None, 0, None, 0) and a[25] and a[26] is None
            assert b[16:18] == (2, 3) and b[18:21] == (7001, 64, 7002)
            assert b[21] and b[22] == 640 and b[23] == block.data_ptr() and b[24] == 5 and b[25] is None and b[26] is None
            assert len(a) == len(b) == 27
            # nothing fed back (the weight gradient's tile is part of the head), and a plan without a split: the existing block serves,
            # no tensor is created
            L = _PlanRecorder((1, 1, 0, 0))
            with Ops() as ops:
                detmode.plan_launch(L, "omni_conv2d_wgrad_det", like, head)
            assert ops.seen == []
            (n0, a), (n1, b) = L.calls
            assert n0 == n1 == "omni_conv2d_wgrad_det" and a[:16] == b[:16] == head
            assert a[16:20] == (None, 0, None, 0) and a[20] and a[21] is None
            assert b[16:] == (None, 0, block.data_ptr(), 1, None, None)
            # workspace-only tail of the stem weight gradients: at least one float behind a non-null pointer, the reported size passed on
            for floats in (0, 100):
                L = _PlanRecorder((0, 0, 0, floats))
                detmode.plan_launch(L, "omni_stem_conv_wgrad_det", like, head[:12], counters=False)
                (n0, a), (n1, b) = L.calls
                assert n0 == n1 == "omni_stem_conv_wgrad_det" and a[:12] == b[:12] == head[:12]
                assert a[12:14] == (None, 0) and a[14] and a[15] is None
                assert b[12] and b[13:] == (floats, None, None)
        finally:
            detmode._counters.pop(detmode._key(like), None)


def _step_outputs(model, batch, E, gold):
    from omni3d_amd.d2.events import EventStorage
    model.proposal_generator.injected = {"E": E["rpn"], "proposals": gold["proposals"]}
    model.roi_heads.injected = {"E": E["roi"]}
    for p in model.parameters():
        p.grad = None
    model.train()
    with EventStorage(0):
        losses = model(batch)
        sum(losses.values()).backward()
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in losses.items()}, {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dla34_full", "resnet34_full"])
def test_training_step_is_bit_identical_run_to_run_gpu(hip_lib, name):
    """the whole step -- forward, ten losses, backward -- twice on the same weights, batch and sampling variates"""
    from oracle import make_golden as MG
    from omni3d_amd import synthetic
    from omni3d_amd.kernels import detmode
    assert detmode.on(), "the deterministic reductions are the shipped default"
    gold = torch.load(os.path.join(ROOT, "tests", "golden", name + ".pt"), weights_only=False)
    spec = gold["spec"]
    priors = synthetic.make_priors(50, bins=spec.get("prior_bins", 0))
    model = MG.build_product_model(MG.product_cfg(spec["overrides"], spec.get("config", "cubercnn_DLA34_FPN.yaml")), priors, spec["seed"], device="cuda")
    batch = synthetic.make_batch(spec["images"], spec["height"], spec["width"], num_gt=spec["num_gt"], seed=spec["seed"], priors=priors)
    E = MG.variates(spec, gold["rpn_labels"].shape[1])
    bufs = [b.detach().clone() for b in model.buffers()]
    runs = []
    for _ in range(3):
        with torch.no_grad():
            for b, s in zip(model.buffers(), bufs):         # BatchNorm running statistics back to the start
                b.copy_(s)
        runs.append(_step_outputs(model, batch, E, gold))
    l0, g0 = runs[0]
    for li, gi in runs[1:]:
        for k in l0:
            assert torch.equal(l0[k], li[k]), (k, float(l0[k]), float(li[k]))
        assert set(g0) == set(gi)
        bad = [n for n in g0 if not torch.equal(g0[n], gi[n])]
        assert not bad, (len(bad), bad[:8])
    # every arrival counter the three steps used is back at zero (csrc/split_reduce.h: the protocol's invariant)
    assert detmode.nonzero_counters() == []


@pytest.mark.gpu
def test_split_reduce_memory_ordering_litmus_gpu(hip_lib):
    """csrc/split_reduce.h publishes a split's partial tile with agent-scope (sc1) stores, waits for them (s_waitcnt
    vmcnt(0)), takes a ticket with a relaxed atomic and lets the LAST arrival read every slot -- ordering by control dependency, no
    release / acquire fences.  The litmus: many-way split reductions whose splits land on different XCDs (different, non-coherent
    L2s), hammered 300 times each; a slot read that overtook its store would show up as a result that differs from the first run
    (the sum is order-fixed, so ANY difference is a stale read) or as a counter left behind."""
    from omni3d_amd.kernels import conv, detmode
    assert detmode.on()
    g = torch.Generator().manual_seed(11)
    cases = [  # few tiles, deep reductions: every tile is met by 8-32 workgroups
        ((2, 512, 8, 8), (256, 512, 3, 3), 1, 1, 16),       # 2 x 4 tiles x 16 splits
        ((1, 256, 6, 6), (64, 256, 3, 3), 1, 1, 32),        # one row of tiles x 32 splits: the two-level (grouped) reduction
        ((4, 128, 16, 16), (128, 128, 1, 1), 1, 0, 4),
    ]
    for xs, ws, stride, pad, splits in cases:
        x = _cl(torch.randn(*xs, generator=g)).cuda()
        w = _cl(torch.randn(*ws, generator=g) * 0.05).cuda()
        dy = _cl(torch.randn(xs[0], ws[0], xs[2], xs[3], generator=g)).cuda()
        ref_f = conv.conv2d_fwd(x, w, None, stride, pad, tile=2, splits=splits).clone()
        ref_d = conv.conv2d_dgrad(dy, w, (xs[2], xs[3]), stride, pad, tile=2, splits=splits).clone()
        ref_w = conv.conv2d_wgrad(x, dy, (ws[2], ws[3]), stride, pad).clone()
        for it in range(300):
            assert torch.equal(conv.conv2d_fwd(x, w, None, stride, pad, tile=2, splits=splits), ref_f), (xs, "fwd", it)
            assert torch.equal(conv.conv2d_dgrad(dy, w, (xs[2], xs[3]), stride, pad, tile=2, splits=splits), ref_d), (xs, "dgrad", it)
            assert torch.equal(conv.conv2d_wgrad(x, dy, (ws[2], ws[3]), stride, pad), ref_w), (xs, "wgrad", it)
    torch.cuda.synchronize()
    assert detmode.nonzero_counters() == []
