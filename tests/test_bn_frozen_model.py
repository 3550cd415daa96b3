"""A training step with every BatchNorm frozen (freeze_bn after .train(): MODEL.USE_BN False, tools/train_net.py:150-151 of the
reference) against the CPU oracle frozen the same way, in fp32 and in float64 -- losses and every gradient judged like
tests/test_model_parity.py `_vs_cpu_oracle` -- and through the drop-in loop's staged-graph replay (cubercnn/solver/autoreplay.py)."""
import pytest
import torch

import test_model_parity as P


def _frozen_vs_cpu_oracle(batch, config, backbone):
    from oracle import make_golden as MG
    from oracle import model_oracle as MO
    from omni3d_amd import synthetic
    from omni3d_amd.cubercnn.solver.build import freeze_bn
    priors = synthetic.make_priors(50)
    model = MG.build_product_model(MG.product_cfg([], config), priors, 5, device="cpu")
    oracle = MO.ModelOracle(priors, backbone=backbone)
    oracle.load_state_dict(model.state_dict(), strict=True)
    B = len(batch)
    Hp = -(-max(b["image"].shape[1] for b in batch) // 64) * 64
    Wp = -(-max(b["image"].shape[2] for b in batch) // 64) * 64
    A = 3 * sum((Hp // s) * (Wp // s) for s in (4, 8, 16, 32, 64))
    g = torch.Generator().manual_seed(3)
    E_rpn, E_roi = torch.empty(B, A).exponential_(generator=g), torch.empty(B, 2048).exponential_(generator=g)
    # non-trivial running statistics: a few training-mode passes without gradients
    oracle.train()
    with torch.no_grad():
        for _ in range(3):
            oracle(batch, E_rpn, E_roi)
    model.load_state_dict(oracle.state_dict(), strict=True)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to("cuda")
    model.train()
    freeze_bn(model)
    oracle.train()
    freeze_bn(oracle)
    ref = oracle(batch, E_rpn, E_roi)
    sum(ref.values()).backward()
    # the float64 yardstick: oracle/model_oracle.run_fp64, frozen after its .train()
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        o64 = MO.ModelOracle(priors, backbone=backbone)
        o64.load_state_dict(state, strict=True)
        o64 = o64.double()
        o64.train()
        freeze_bn(o64)
        l64 = o64(MO.to_double(batch), E_rpn.double(), E_roi.double(), proposals=[p.double() for p in oracle.last_proposals])
        sum(l64.values()).backward()
    finally:
        torch.set_default_dtype(prev)
    l64 = {k: float(v.detach()) for k, v in l64.items()}
    g64 = {n: p.grad for n, p in o64.named_parameters() if p.grad is not None}
    assert torch.equal(o64.last_labels, oracle.last_labels)
    model.proposal_generator.injected = {"E": E_rpn, "proposals": oracle.last_proposals}
    model.roi_heads.injected = {"E": E_roi}
    bufs = {n: b.clone() for n, b in model.named_buffers()}
    losses = model(batch)
    sum(losses.values()).backward()
    for n, b in model.named_buffers():          # running statistics and num_batches_tracked untouched
        assert torch.equal(b, bufs[n]), n
    assert torch.equal(model.proposal_generator.last_labels.cpu(), oracle.last_labels)
    for got, cls, want in zip(model.roi_heads.last_sampled_boxes.cpu(), model.roi_heads.last_sampled_classes.cpu(), oracle.last_roi_boxes):
        got = got[cls >= 0]
        assert len(got) == len(want)
        d = (got[:, None, :] - want[None, :, :]).abs().amax(dim=2)
        assert float(d.min(dim=1).values.max()) <= 1e-3 and float(d.min(dim=0).values.max()) <= 1e-3
    bad = []
    for k, v64 in l64.items():
        hip, cpu = float(losses[k].detach()), float(ref[k].detach())
        scale = max(1.0, abs(v64))
        e_hip, e_cpu = abs(hip - v64) / scale, abs(cpu - v64) / scale
        if not (e_hip <= P.LOSS_ABS and e_hip <= max(2 * e_cpu, P.LOSS_FLOOR)):
            bad.append(("loss", k, v64, e_hip, e_cpu))
    og = dict(oracle.named_parameters())
    n_rule = n_all = 0
    for n, p in model.named_parameters():
        if not p.requires_grad:
            continue
        if n.startswith("backbone.bottom_up.") and n in g64:     # the trunk learns (the reference's dropped projections excepted)
            assert p.grad is not None and float(p.grad.abs().max()) > 0, ("no gradient", n)
        if p.grad is None:
            continue
        if n not in g64:
            continue
        den = float(g64[n].norm().clamp(min=1e-30))
        gh = p.grad.detach().double().cpu()
        if gh.dim() == 4:
            gh = gh.contiguous(memory_format=torch.contiguous_format)
        e_hip = float((gh.reshape(g64[n].shape) - g64[n]).norm()) / den
        e_cpu = float((og[n].grad.double() - g64[n]).norm()) / den
        if den < 1e-12:
            continue
        n_all += 1
        n_rule += e_hip <= max(P.GRAD_RULE_MULT * e_cpu, P.GRAD_FLOOR)
        if not e_hip <= (P.GRAD_CAP_HEADS if P._is_head(n) else P.GRAD_CAP_BACKBONE):
            bad.append(("grad", n, e_hip, e_cpu))
    assert n_all > 0 and n_rule >= P.GRAD_RULE_FRACTION * n_all, (n_rule, n_all)
    assert not bad, bad[:20]
    # deterministic: a second run of the step gives the same gradients
    first = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    for p in model.parameters():
        p.grad = None
    sum(model(batch).values()).backward()
    for n, p in model.named_parameters():
        if n in first:
            assert torch.equal(first[n], p.grad), n


@pytest.mark.gpu
def test_frozen_bn_step_dla34_vs_cpu_oracle(hip_lib):
    from omni3d_amd import synthetic
    priors = synthetic.make_priors(50)
    _frozen_vs_cpu_oracle(synthetic.make_batch(2, 128, 128, num_gt=6, seed=51, priors=priors), "cubercnn_DLA34_FPN.yaml", "dla34")


@pytest.mark.gpu
def test_frozen_bn_step_resnet34_vs_cpu_oracle(hip_lib):
    from omni3d_amd import synthetic
    priors = synthetic.make_priors(50)
    _frozen_vs_cpu_oracle(synthetic.make_batch(2, 128, 128, num_gt=6, seed=53, priors=priors), "cubercnn_ResNet34_FPN.yaml", "resnet34")


def _set_running_stats(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)


SMALL = ["MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", 64, "MODEL.RPN.BATCH_SIZE_PER_IMAGE", 64, "MODEL.RPN.PRE_NMS_TOPK_TRAIN", 300,
         "MODEL.RPN.POST_NMS_TOPK_TRAIN", 100, "SOLVER.BASE_LR", 0.0002]


def _close_logs(log_a, log_b, tol):
    # (tolerances of tests/test_autoreplay.py: the staged backward sums the gradients that meet at its cut tensors in another order)
    for it, (a, b) in enumerate(zip(log_a, log_b)):
        assert set(a) == set(b)
        t = tol if it < 2 else 10 * tol
        for k in a:
            assert abs(a[k] - b[k]) <= t * max(1.0, abs(b[k])), (it, k, a[k], b[k])


@pytest.mark.gpu
def test_frozen_bn_dropin_loop_replay_gpu(hip_lib):
    """the reference loop with freeze_bn(model): captured and replayed frozen steps train like eager launches and leave the running
    statistics alone"""
    import test_autoreplay as T
    from omni3d_amd.cubercnn.solver.build import freeze_bn
    runs = []
    for replay in (True, False):
        model, opt, pool = T._build("cuda", SMALL, 128)
        _set_running_stats(model, 1)
        if not replay:
            model.__dict__["_omni_auto"] = None
        else:
            model._omni_auto.warm = 1
        freeze_bn(model)
        bufs = [b.clone() for b in model.buffers()]
        start = opt.flat_param.clone()
        log = T._loop(model, opt, pool, 4)
        assert all(torch.equal(a, b) for a, b in zip(bufs, model.buffers()))
        runs.append((model, opt, log, start))
    (ma, oa, la, start), (mb, ob, lb, _) = runs
    auto = ma._omni_auto
    assert auto.failed is None and auto.replays == 3, (auto.failed, auto.replays)
    _close_logs(la, lb, 1e-3)
    d = float((oa.flat_param - ob.flat_param).abs().max())
    moved = float((ob.flat_param - start).abs().max())
    assert moved > 0 and d <= 0.15 * moved, (d, moved)


@pytest.mark.gpu
def test_frozen_bn_after_capture_does_not_replay_stale_step_gpu(hip_lib):
    """capture with BatchNorm training, then freeze_bn: the next steps are frozen steps (eager, then a fresh capture), not replays of
    the batch-statistics graph"""
    import test_autoreplay as T
    from omni3d_amd.cubercnn.solver.build import freeze_bn
    runs = []
    for replay in (True, False):
        model, opt, pool = T._build("cuda", SMALL, 128)
        if not replay:
            model.__dict__["_omni_auto"] = None
        else:
            model._omni_auto.warm = 1
        log = T._loop(model, opt, pool[:1], 2)
        if replay:
            assert model._omni_auto.replays == 1 and len(model._omni_auto.cache) == 1
        freeze_bn(model)
        bufs = [b.clone() for b in model.buffers()]
        log += T._loop(model, opt, pool[:1], 3, seed=1)
        assert all(torch.equal(a, b) for a, b in zip(bufs, model.buffers()))     # a stale replay would move the running statistics
        runs.append((model, opt, log))
    (ma, oa, la), (mb, ob, lb) = runs
    auto = ma._omni_auto
    assert auto.failed is None and auto.captures == 2 and auto.replays == 3, (auto.failed, auto.captures, auto.replays)
    _close_logs(la, lb, 1e-3)
