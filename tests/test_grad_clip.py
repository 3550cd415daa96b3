"""SOLVER.CLIP_GRADIENTS (detectron2 maybe_add_gradient_clipping, applied last by cubercnn/solver/build.py:68): the fused per-parameter
clip of the flat-bucket optimizers (csrc/optim.hip omni_clip_norm_* / omni_*_step_clipped) against torch itself -- per-parameter
torch.nn.utils.clip_grad_norm_ / clip_grad_value_, then torch.optim.SGD / Adam / AdamW on a copy; norms against float64."""
import sys

import pytest
import torch
from torch import nn

from conftest import ROOT

INF = float("inf")
ADAM_TYPES = ["adam", "adam+amsgrad", "adamw", "adamw+amsgrad"]


def _cfg(*overrides):
    from omni3d_amd.cubercnn.config import get_cfg_defaults
    from omni3d_amd.d2.config import get_cfg
    cfg = get_cfg()
    get_cfg_defaults(cfg)
    cfg.merge_from_list(list(overrides))
    return cfg


def _clip_cfg(clip_type, value, norm_type=2.0):
    return _cfg("SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", clip_type,
                "SOLVER.CLIP_GRADIENTS.CLIP_VALUE", value, "SOLVER.CLIP_GRADIENTS.NORM_TYPE", norm_type)


def _torch_clip(params, clip):
    """the reference's per-parameter clipper (detectron2 _create_gradient_clipper) on torch's own functions"""
    kind, value, norm_type = clip
    for p in params:
        if kind == "norm":
            torch.nn.utils.clip_grad_norm_(p, value, norm_type)
        else:
            torch.nn.utils.clip_grad_value_(p, value)


# ---- optimizers over a set of parameters of given sizes -------------------------------------------------------------------------
def _make(sizes, kind, dev, seed=0):
    """(flat optimizer, its parameters), (torch optimizer, its parameters): same initial values, alternating groups"""
    from omni3d_amd.cubercnn.solver.build import FlatAdam, FlatSGD
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(s, generator=g) for s in sizes]
    a = [nn.Parameter(t.clone().to(dev)) for t in init]
    b = [nn.Parameter(t.clone().to(dev)) for t in init]

    def groups(ps):
        return [{"params": [p], "lr": 0.05 if i % 2 else 0.02, "weight_decay": (1e-2, 0.0, 3e-2)[i % 3]} for i, p in enumerate(ps)]
    if kind == "sgd":
        fo = FlatSGD(groups(a), 0.02, momentum=0.9, direct_accumulate=False)
        to = torch.optim.SGD(groups(b), 0.02, momentum=0.9)
    else:
        ams, adamw = kind.endswith("+amsgrad"), kind.startswith("adamw")
        fo = FlatAdam(groups(a), 0.02, eps=1e-2, amsgrad=ams, decoupled=adamw, direct_accumulate=False)
        to = (torch.optim.AdamW if adamw else torch.optim.Adam)(groups(b), 0.02, eps=1e-2, amsgrad=ams)
    return fo, a, to, b


def _grads(sizes, it, dev, scales):
    g = torch.Generator().manual_seed(100 + it)
    return [(torch.randn(s, generator=g) * sc).to(dev) for s, sc in zip(sizes, scales)]


def _run(sizes, kind, clip, dev, steps=5, scales=None, grad_scale=1.0, tol=2e-6):
    """`steps` updates of the fused clip against torch's per-parameter clip + torch's optimizer; -> (fo, a, to, b, #clipped)"""
    fo, a, to, b = _make(sizes, kind, dev)
    if clip is not None:
        fo.arm_clipping(*clip)
    scales = scales or [(0.1, 3.0, 30.0)[i % 3] for i in range(len(sizes))]
    clipped = 0
    for it in range(steps):
        gs = _grads(sizes, it, dev, scales)
        fo.zero_grad()
        to.zero_grad()
        for p, q, gr in zip(a, b, gs):
            p.grad.copy_(gr / grad_scale)          # a summing exchange left world x the average behind
            q.grad = gr.clone()
        fo._grad_scale = grad_scale
        if clip is not None:
            if clip[0] == "norm":
                clipped += sum(float(torch.linalg.vector_norm(q.grad.double(), clip[2])) > clip[1] for q in b)
            else:
                clipped += sum(float(q.grad.abs().max()) > clip[1] for q in b)
            _torch_clip(b, clip)
        fo.step()
        to.step()
        for i, (p, q) in enumerate(zip(a, b)):
            d = float((p.detach() - q.detach()).abs().max())
            assert d <= tol, (kind, clip, it, i, d)
    return fo, a, to, b, clipped


SIZES = [1, 3, 4, 5, 65537, 3 * 8192 + 7]


@pytest.mark.parametrize("norm_type", [1.0, 2.0, INF, 3.0])
def test_clip_norms_match_float64_emulated(emu_lib, norm_type):
    """per-parameter norms over a ragged tile table (1, 3, 4, 5 elements, 65 537, one parameter of several tiles), with and without
    the deferred 1/world"""
    from omni3d_amd.kernels import det
    assert SIZES[-1] > 3 * det.CLIP_TILE
    fo, a, _, _ = _make(SIZES, "sgd", "cpu")
    fo.arm_clipping("norm", 1.0, norm_type)
    assert fo._clip_t["tiles"].shape[0] == 4 + 9 + 4
    for scale in (1.0, 0.5):
        for p, g in zip(a, _grads(SIZES, 0, "cpu", [3.0] * len(SIZES))):
            p.grad.copy_(g)
        fo._grad_scale = scale
        fo._clip_norm_pass()
        ref = torch.stack([torch.linalg.vector_norm(p.grad.double() * scale, norm_type) for p in a])
        rel = ((fo.clip_norms.double() - ref).abs() / ref).max()
        assert float(rel) <= 1e-6, (norm_type, scale, float(rel))
        coef = torch.clamp(1.0 / (fo.clip_norms + 1e-6), max=1.0)
        assert torch.equal(fo._clip_t["coef"], coef)


@pytest.mark.parametrize("kind", ["sgd"] + ADAM_TYPES)
@pytest.mark.parametrize("clip", [("norm", 2.0, 2.0), ("norm", 1.0, INF), ("norm", 5.0, 1.0), ("value", 0.5, 2.0)])
def test_clipped_optimizers_match_torch_emulated(emu_lib, kind, clip):
    *_, clipped = _run([7, 64, 1, 300, 5, 33], kind, clip, "cpu")
    assert 0 < clipped < 5 * 6 or clip[0] == "value", clipped        # some parameters clip, some do not


def test_clip_uses_the_averaged_gradient_emulated(emu_lib):
    """_grad_scale = 1/world (all_reduce_finish(defer_scale=True)): norms and clamps are those of the averaged gradient"""
    for clip in (("norm", 2.0, 2.0), ("value", 0.5, 2.0)):
        _run([7, 64, 1, 300, 5, 33], "sgd", clip, "cpu", grad_scale=0.5)
        _run([7, 64, 1, 300, 5, 33], "adamw", clip, "cpu", grad_scale=0.5)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_nonfinite_gradients_propagate_like_torch_emulated(emu_lib, kind):
    """MODEL.STABILIZE 0 (no guard): a NaN makes its parameter's norm and coefficient NaN, an Inf makes the coefficient 0 (inf * 0 =
    NaN in that element); the value clamp keeps NaN and clamps Inf"""
    sizes = [6, 9, 5]
    for clip in (("norm", 1.0, 2.0), ("norm", 1.0, INF), ("value", 0.5, 2.0)):
        fo, a, to, b = _make(sizes, kind, "cpu")
        fo.arm_clipping(*clip)
        gs = _grads(sizes, 0, "cpu", [2.0, 2.0, 2.0])
        gs[0][2] = float("nan")
        gs[1][4] = INF
        for p, q, gr in zip(a, b, gs):
            p.grad.copy_(gr)
            q.grad = gr.clone()
        _torch_clip(b, clip)
        fo.step()
        to.step()
        for p, q in zip(a, b):
            torch.testing.assert_close(p.detach(), q.detach(), atol=2e-6, rtol=0, equal_nan=True)
        assert bool(torch.isnan(a[0]).any()) and not bool(torch.isnan(a[2]).any())


def _fused_head(dev):
    from omni3d_amd.cubercnn.modeling.roi_heads.fast_rcnn import FastRCNNOutputs
    torch.manual_seed(4)
    head = FastRCNNOutputs(64, box2box_weights=(10.0, 10.0, 5.0, 5.0), num_classes=50).to(dev)
    for p in head.parameters():
        p.data.normal_(0, 0.1)
    return head


def _run_fused_groups(dev):
    """cls_score + bbox_pred sit back to back in the bucket (the biases at unaligned offsets): each member clips on its own norm"""
    import copy
    from omni3d_amd.cubercnn.solver.build import FlatSGD, fused_view, tag_fused_groups
    head = _fused_head(dev)
    ref = copy.deepcopy(head)
    tag_fused_groups(head)
    opt = FlatSGD([{"params": [p]} for p in head.parameters()], lr=0.1, momentum=0.9, weight_decay=1e-3)
    assert fused_view([head.cls_score.bias, head.bbox_pred.bias], True) is not None
    opt.arm_clipping("norm", 0.5, 2.0)
    opt_r = torch.optim.SGD(ref.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-3)
    clipped = 0
    for it in range(3):
        g = torch.Generator().manual_seed(it)
        grads = [(torch.randn(p.shape, generator=g) * (0.01 if i % 2 else 1.0)).to(dev) for i, p in enumerate(ref.parameters())]
        opt.zero_grad()
        for p, q, gr in zip(head.parameters(), ref.parameters(), grads):
            p.grad.copy_(gr)
            q.grad = gr.clone()
        norms = [float(q.grad.norm()) for q in ref.parameters()]
        clipped += sum(n > 0.5 for n in norms)
        _torch_clip(list(ref.parameters()), ("norm", 0.5, 2.0))
        opt.step()
        opt_r.step()
        assert torch.allclose(opt.clip_norms.cpu(), torch.tensor(norms), rtol=1e-6, atol=0)
        for (n, p), (_, q) in zip(head.named_parameters(), ref.named_parameters()):
            assert float((p.data - q.data).abs().max()) <= 2e-6, (it, n)
    assert 0 < clipped < 3 * len(norms)
    # the zero padding of the fused groups is left alone
    fw = fused_view([head.cls_score.weight, head.bbox_pred.weight], True)
    assert float(fw[0][251 * 64:].abs().max()) == 0.0


def test_fused_groups_clip_each_member_emulated(emu_lib):
    _run_fused_groups("cpu")


# ---- build_optimizer / maybe_add_gradient_clipping ---------------------------------------------------------------------------------
def _net():
    torch.manual_seed(0)
    return nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4), nn.Conv2d(4, 2, 1))


def _train(opt, net, steps=3, scale=20.0):
    for it in range(steps):
        g = torch.Generator().manual_seed(it)
        x = torch.randn(2, 3, 6, 6, generator=g)
        opt.zero_grad()
        ((net(x) ** 2).mean() * scale).backward()
        opt.step()


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_build_optimizer_honours_clip_gradients_emulated(emu_lib, kind):
    from omni3d_amd.cubercnn.solver import build_optimizer
    from omni3d_amd.d2.solver import maybe_add_gradient_clipping
    cfg = _clip_cfg("norm", 0.05, 2.0)
    cfg.SOLVER.TYPE = kind
    net_a, net_b = _net(), _net()
    opt = build_optimizer(cfg, net_a)
    assert opt.clip == ("norm", 0.05, 2.0)
    # the reference's form: the same parameter groups in torch's optimizer, class-swapped by the same function
    from omni3d_amd.cubercnn.solver.build import _param_groups
    groups = _param_groups(cfg, net_b)
    ref = torch.optim.SGD(groups, cfg.SOLVER.BASE_LR, momentum=cfg.SOLVER.MOMENTUM) if kind == "sgd" else \
        torch.optim.AdamW(groups, cfg.SOLVER.BASE_LR, eps=1e-2)
    ref = maybe_add_gradient_clipping(cfg, ref)
    assert type(ref).__name__ == ("SGD" if kind == "sgd" else "AdamW") + "WithGradientClip"
    _train(opt, net_a)
    _train(ref, net_b)
    for p, q in zip(net_a.parameters(), net_b.parameters()):
        assert float((p.detach() - q.detach()).abs().max()) <= 2e-6
    # and clipping did something: the unclipped run lands elsewhere
    cfg.SOLVER.CLIP_GRADIENTS.ENABLED = False
    net_c = _net()
    _train(build_optimizer(cfg, net_c), net_c)
    assert max(float((p - q).abs().max()) for p, q in zip(net_a.parameters(), net_c.parameters())) > 1e-4


def test_unknown_clip_type_raises(emu_lib):
    from omni3d_amd.cubercnn.solver import build_optimizer
    from omni3d_amd.d2.solver import GradientClipType, maybe_add_gradient_clipping
    with pytest.raises(ValueError):
        build_optimizer(_clip_cfg("full_model", 1.0), _net())
    with pytest.raises(ValueError):
        maybe_add_gradient_clipping(_clip_cfg("l2", 1.0), torch.optim.SGD(_net().parameters(), 0.1))
    assert GradientClipType("norm") is GradientClipType.NORM and GradientClipType("value") is GradientClipType.VALUE


def test_disabled_returns_the_optimizer_unchanged():
    from omni3d_amd.d2.solver import maybe_add_gradient_clipping
    opt = torch.optim.SGD(_net().parameters(), 0.1)
    assert maybe_add_gradient_clipping(_cfg(), opt) is opt and type(opt) is torch.optim.SGD
    assert maybe_add_gradient_clipping(_cfg(), torch.optim.Adam) is torch.optim.Adam
    cls = maybe_add_gradient_clipping(_clip_cfg("value", 0.1), torch.optim.Adam)
    assert issubclass(cls, torch.optim.Adam) and cls.__name__ == "AdamWithGradientClip"


def test_flat_optimizer_class_form_arms_the_fused_clip(emu_lib):
    from omni3d_amd.cubercnn.solver.build import FlatSGD
    from omni3d_amd.d2.solver import maybe_add_gradient_clipping
    cls = maybe_add_gradient_clipping(_clip_cfg("value", 0.25), FlatSGD)
    opt = cls(_net().parameters(), 0.1, momentum=0.9)
    assert isinstance(opt, FlatSGD) and opt.clip == ("value", 0.25, 2.0)


def _launches(emu_lib, monkeypatch, cfg, kind):
    from omni3d_amd.cubercnn.solver import build_optimizer
    cfg.SOLVER.TYPE = kind
    net = _net()
    opt = build_optimizer(cfg, net)
    _train(opt, net, steps=1)
    names = []
    real = emu_lib.call
    monkeypatch.setattr(emu_lib, "call", lambda name, *args: (names.append(name), real(name, *args))[1])
    opt.step()
    monkeypatch.undo()
    return names, len(opt.segments)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_launch_sequence(emu_lib, monkeypatch, kind):
    """ENABLED False: exactly today's launches; norm: two more (the norm pass), value: none more"""
    upd = "omni_sgd_step" if kind == "sgd" else "omni_adam_step"
    tick = [] if kind == "sgd" else ["omni_adam_tick"]
    names, nseg = _launches(emu_lib, monkeypatch, _cfg(), kind)
    assert names == tick + [upd] * nseg, names
    names, nseg = _launches(emu_lib, monkeypatch, _clip_cfg("norm", 1.0), kind)
    assert names == ["omni_clip_norm_partials", "omni_clip_norm_coef"] + tick + [upd + "_clipped"] * nseg, names
    names, nseg = _launches(emu_lib, monkeypatch, _clip_cfg("value", 1.0), kind)
    assert names == tick + [upd + "_clipped"] * nseg, names


@pytest.mark.parametrize("kind", ["sgd"] + ADAM_TYPES)
def test_huge_clip_value_is_bit_identical_to_disabled_emulated(emu_lib, kind):
    """a coefficient of exactly 1 is a no-op: CLIP_VALUE 1e30 trains the same bits as no clipping"""
    sizes = [7, 64, 1, 300, 5, 33]
    fo, a, *_ = _run(sizes, kind, ("norm", 1e30, 2.0), "cpu", tol=INF)
    fo2, a2, *_ = _run(sizes, kind, None, "cpu", tol=INF)
    assert torch.equal(fo.flat_param, fo2.flat_param)
    assert all(torch.equal(fo.flat_state[k], fo2.flat_state[k]) for k in fo.STATE)


def test_skip_flag_gates_the_clipped_update_emulated(emu_lib):
    for kind in ("sgd", "adam"):
        for clip in (("norm", 1.0, 2.0), ("value", 0.5, 2.0)):
            fo, a, _, _ = _make([7, 64, 1], kind, "cpu")
            fo.arm_clipping(*clip)
            fo.skip_flag = torch.ones(1)
            for p in a:
                p.grad.fill_(3.0)
            before = fo.flat_param.clone()
            fo.step()
            assert torch.equal(fo.flat_param, before)


def test_alias_detectron2_solver_build():
    """the reference's own build.py imports `from detectron2.solver.build import maybe_add_gradient_clipping` (:4)"""
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); import omni3d_amd; omni3d_amd.install()\n"
            "from detectron2.solver.build import maybe_add_gradient_clipping\n"
            "import omni3d_amd.d2.solver as S; assert maybe_add_gradient_clipping is S.maybe_add_gradient_clipping; print('OK')") % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stderr[-2000:]


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
GPU_SIZES = [12544 * 1024, 1, 1024, 1, 3, 12544 * 1024 // 7 + 5, 1]


@pytest.mark.gpu
def test_clip_norms_match_float64_gpu(hip_lib):
    from omni3d_amd.kernels import det
    fo, a, _, _ = _make(GPU_SIZES, "sgd", "cuda")
    for norm_type in (1.0, 2.0, INF, 3.0):
        fo.arm_clipping("norm", 1.0, norm_type)
        for scale in (1.0, 0.5):
            for p, g in zip(a, _grads(GPU_SIZES, 0, "cuda", [3.0] * len(GPU_SIZES))):
                p.grad.copy_(g)
            fo._grad_scale = scale
            fo._clip_norm_pass()
            ref = torch.stack([torch.linalg.vector_norm(p.grad.double() * scale, norm_type) for p in a])
            rel = ((fo.clip_norms.double() - ref).abs() / ref).max()
            assert float(rel) <= 1e-6, (norm_type, scale, float(rel))
    assert fo._clip_t["tiles"].shape[0] > 12544 * 1024 // det.CLIP_TILE


@pytest.mark.gpu
def test_clipped_optimizers_match_torch_gpu(hip_lib):
    """a 12 544 x 1024 parameter (the box head's fc1) next to one-element ones"""
    scales = [1e-3, 10.0, 0.1, 1e-6, 5.0, 1e-3, 0.3]
    for kind in ["sgd"] + ADAM_TYPES:
        for clip in (("norm", 1.0, 2.0), ("norm", 0.5, INF), ("value", 0.5, 2.0)):
            *_, clipped = _run(GPU_SIZES, kind, clip, "cuda", steps=3, scales=scales, grad_scale=0.5 if kind == "adamw" else 1.0)
            assert clipped > 0
        # a coefficient of 1 is an exact no-op on the gradient; the clipped update kernel's fused multiply-adds may pair the products
        # differently from the unclipped one's on gfx950 (the host build contracts nothing and is bit-identical, see above): last bit
        fo, *_ = _run(GPU_SIZES, kind, ("norm", 1e30, 2.0), "cuda", steps=3, scales=scales, tol=INF)
        fo2, *_ = _run(GPU_SIZES, kind, None, "cuda", steps=3, scales=scales, tol=INF)
        err = (fo.flat_param - fo2.flat_param).abs() / fo2.flat_param.abs().clamp(min=1.0)
        assert float(err.max()) <= 1e-6, (kind, float(err.max()))


@pytest.mark.gpu
def test_fused_groups_clip_each_member_gpu(hip_lib):
    _run_fused_groups("cuda")


CLIP = ("norm", 0.02, 2.0)
SMALL = ["MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", 64, "MODEL.RPN.BATCH_SIZE_PER_IMAGE", 64, "MODEL.RPN.PRE_NMS_TOPK_TRAIN", 300,
         "MODEL.RPN.POST_NMS_TOPK_TRAIN", 100, "SOLVER.BASE_LR", 0.0002, "MODEL.STABILIZE", 0.0,
         "SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", CLIP[0], "SOLVER.CLIP_GRADIENTS.CLIP_VALUE", CLIP[1],
         "SOLVER.CLIP_GRADIENTS.NORM_TYPE", CLIP[2]]


def _span(opt, p):
    off, n = opt._slot[id(p)]
    return off, off + n


def _dla_run(replay, iters=8):
    """DLA-34 at the small fixture configuration through the reference's loop body (model(data) / zero_grad / backward / step).  Every
    step is checked against torch's per-parameter clip + torch.optim.SGD applied to a snapshot of the same flat gradient."""
    from test_autoreplay import _build, _loop
    from omni3d_amd.cubercnn.solver.build import FlatSGD
    model, opt, pool = _build("cuda", SMALL, 128)
    assert isinstance(opt, FlatSGD) and opt.clip == CLIP
    auto = model._omni_auto
    if replay:
        auto.warm = 1
    else:
        model.__dict__["_omni_auto"] = None
    params = opt._ordered_params()
    stats = {"clipped": [], "worst": 0.0}
    step = opt.step

    def checked_step(closure=None):
        torch.cuda.synchronize()
        first = opt._steps == 0
        snap = [(p.detach().clone(), opt._view_like(opt.flat_grad[slice(*_span(opt, p))], p).clone(),
                 opt._state_view("momentum_buffer", p).detach().clone()) for p in params]
        step()
        torch.cuda.synchronize()
        groups = {id(p): g for g in opt.param_groups for p in g["params"]}
        clipped = 0
        for p, (p0, g0, m0) in zip(params, snap):
            holder = nn.Parameter(torch.empty_like(g0))
            holder.grad = g0 * opt._grad_scale
            clipped += float(torch.linalg.vector_norm(holder.grad.double(), CLIP[2])) > CLIP[1]
            torch.nn.utils.clip_grad_norm_(holder, CLIP[1], CLIP[2])
            g = groups[id(p)]
            d = holder.grad + g["weight_decay"] * p0
            m = d if first else g["momentum"] * m0 + d
            want = p0 - g["lr"] * m
            err = (p.detach() - want).abs() / want.abs().clamp(min=1.0)        # 2e-6, relative above magnitude 1 (fp32 ulp)
            stats["worst"] = max(stats["worst"], float(err.max()))
        stats["clipped"].append(clipped)

    opt.step = checked_step
    _loop(model, opt, pool, iters)
    if replay:
        assert auto.failed is None and auto.replays == iters - 1, (auto.failed, auto.replays)
    return opt.flat_param.clone(), stats, len(params)


@pytest.mark.gpu
def test_dla34_training_with_norm_clipping_gpu(hip_lib):
    """8 iterations: the first eager, then AutoReplay's staged-graph replay; many parameters clip at CLIP_VALUE 0.02; every step equals
    the torch-clipped reference on its own gradient snapshot; two runs of each form are bit-identical"""
    a, sa, nparams = _dla_run(replay=True)
    assert sa["worst"] <= 2e-6, sa
    assert min(sa["clipped"]) >= nparams // 4, (sa["clipped"], nparams)
    b, sb, _ = _dla_run(replay=True)
    assert torch.equal(a, b) and sa["clipped"] == sb["clipped"]
    c, sc, _ = _dla_run(replay=False)
    assert sc["worst"] <= 2e-6, sc
    d, _, _ = _dla_run(replay=False)
    assert torch.equal(c, d)
