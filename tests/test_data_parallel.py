"""Multi-process data-parallel path on CPU: world_size 2 over gloo.  Each rank runs the
kernels (host-emulated) on its own shard, the flat gradient bucket is all-reduced once and averaged, the
fused SGD step is applied; every rank must end with the parameters of a single process that averaged the
two per-shard gradients itself."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _make_net():
    from omni3d_amd.cubercnn.modeling.layers import BatchNorm2d, Conv2d, FlattenLinear, Linear

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.c = Conv2d(8, 16, 3, padding=1, bias=True)
            self.bn = BatchNorm2d(16)
            self.f = FlattenLinear(16, 4, 12)
            self.l = Linear(12, 8)

        def forward(self, x):
            return self.l(self.f(self.bn(self.c(x, relu=True), relu=True), relu=True)).square().mean()
    torch.manual_seed(0)
    return Net()


def _shard(rank):
    g = torch.Generator().manual_seed(100 + rank)
    return torch.randn(3, 8, 4, 4, generator=g).contiguous(memory_format=torch.channels_last)


def _install_emulator():
    sys.path.insert(0, ROOT)
    from omni3d_amd import lib as L
    L._install_for_tests(L.HipLibrary(os.path.join(ROOT, "tests", "hipemu", "libomni3d_emu.so"), emulated=True))


def _make_cut_net():
    """backbone (conv+bn) | heads (flatten-linear + linear) with the feature cut between them, like RCNN3D.forward"""
    from omni3d_amd.cubercnn.modeling.layers import BatchNorm2d, Conv2d, FlattenLinear, Linear

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.backbone = torch.nn.Module()
            self.backbone.c = Conv2d(8, 16, 3, padding=1, bias=True)
            self.backbone.bn = BatchNorm2d(16)
            self.f = FlattenLinear(16, 4, 12)
            self.l = Linear(12, 8)
            self.feature_cut = None

        def forward(self, x, packed=None):
            feats = {"p": self.backbone.bn(self.backbone.c(x, relu=True), relu=True)}
            if self.feature_cut is not None:
                feats = self.feature_cut(feats)
            return {"loss": self.l(self.f(feats["p"], relu=True)).square().mean()}
    torch.manual_seed(0)
    return Net()


def _tag_early(net):
    for n, p in net.named_parameters():
        p._omni_early_grad = not n.startswith("backbone.")


def _worker_staged_eager(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _install_emulator()
    from omni3d_amd.cubercnn.solver.build import FlatSGD
    from omni3d_amd.cubercnn.solver.graphed import GraphedPipelined
    net = _make_cut_net()
    _tag_early(net)
    opt = FlatSGD([{"params": [p], "weight_decay": 0.0 if p.dim() == 1 else 1e-3} for p in net.parameters()], lr=0.1, momentum=0.9)
    assert opt.stage_ranges.get(0) and any(opt.stage_ranges.get(k) for k in range(1, opt.n_stages))
    stepper = GraphedPipelined(net, opt, _shard(rank), None, graphs=False)
    for _ in range(2):
        _, _, pending = stepper()
        opt.all_reduce_finish(pending)
        opt.step()
    torch.save({n: p.detach().clone() for n, p in net.named_parameters()}, os.path.join(out, f"tp{rank}.pt"))
    dist.destroy_process_group()


def _worker_single_phase(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _install_emulator()
    from omni3d_amd.cubercnn.solver.build import FlatSGD
    net = _make_cut_net()
    opt = FlatSGD([{"params": [p], "weight_decay": 0.0 if p.dim() == 1 else 1e-3} for p in net.parameters()], lr=0.1, momentum=0.9)
    for _ in range(2):
        opt.zero_grad()
        net(_shard(rank))["loss"].backward()
        opt.all_reduce_grads()
        opt.step()
    torch.save({n: p.detach().clone() for n, p in net.named_parameters()}, os.path.join(out, f"sp{rank}.pt"))
    dist.destroy_process_group()


def test_staged_eager_overlapped_exchange_world2(emu_lib, tmp_path):
    """backward cut at the features + all-reduce of the heads' ranges started before the backbone's backward ==
    plain backward + one exchange (same parameters after two SGD steps, on both ranks): GraphedPipelined in its eager form
    on a backbone without cut points"""
    world = 2
    mp.spawn(_worker_staged_eager, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    mp.spawn(_worker_single_phase, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    tp = [torch.load(os.path.join(tmp_path, f"tp{r}.pt")) for r in range(world)]
    sp = [torch.load(os.path.join(tmp_path, f"sp{r}.pt")) for r in range(world)]
    for n in tp[0]:
        assert torch.equal(tp[0][n], tp[1][n]), n
        assert (tp[0][n] - sp[0][n]).abs().max() <= 1e-6 * max(1.0, float(sp[0][n].abs().max())), n


def _flat_opt(net, kind):
    from omni3d_amd.cubercnn.solver.build import FlatAdam, FlatSGD
    groups = [{"params": [p]} for p in net.parameters()]
    if kind == "sgd":
        return FlatSGD(groups, lr=0.1, momentum=0.9, weight_decay=1e-3)
    return FlatAdam(groups, lr=0.02, eps=1e-2, weight_decay=1e-3, amsgrad=kind.endswith("+amsgrad"), decoupled=kind.startswith("adamw"))


def _worker(rank, world, port, out, explicit=True, kind="sgd"):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _install_emulator()
    net = _make_net()
    opt = _flat_opt(net, kind)
    for _ in range(2):
        opt.zero_grad()
        net(_shard(rank)).backward()
        if explicit:
            opt.all_reduce_grads()
        opt.step()          # not explicit: the loop of tools/train_net.py:245-253 -- step() exchanges the bucket itself
    torch.save(opt.flat_param.clone(), os.path.join(out, f"rank{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.parametrize("explicit,kind", [(True, "sgd"), (False, "sgd"), (True, "adam"), (False, "adamw+amsgrad")])
def test_flat_bucket_allreduce_world2(emu_lib, tmp_path, explicit, kind):
    """explicit=False: a loop that never calls the exchange (the reference's relies on DDP hooks, which direct gradient
    accumulation bypasses) still trains identical replicas -- step() averages the bucket when nobody did.  The fused Adam family
    shares the bucket / exchange code of the fused SGD."""
    world, port = 2, _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path), explicit, kind), nprocs=world, join=True)
    got = [torch.load(os.path.join(tmp_path, f"rank{r}.pt")) for r in range(world)]
    assert torch.equal(got[0], got[1])                      # replicas stay identical
    # single-process reference: two replicas (per-shard BN statistics, like the reference's per-GPU BatchNorm),
    # gradients averaged by hand
    nets = [_make_net() for _ in range(world)]
    opts = [_flat_opt(n, kind) for n in nets]
    for _ in range(2):
        for r in range(world):
            opts[r].zero_grad()
            nets[r](_shard(r)).backward()
        avg = (opts[0].flat_grad + opts[1].flat_grad) / world
        for r in range(world):
            opts[r].flat_grad.copy_(avg)
            opts[r].step()
    assert (got[0] - opts[0].flat_param).abs().max() < 1e-6


# ---- the REAL model: tiny cubercnn_DLA34_FPN step over gloo, world 2 (slow under the host emulator) ------------------------
def _tiny_model_and_batch(rank):
    from oracle import make_golden as MG
    from omni3d_amd import synthetic
    spec = MG.TINY
    priors = synthetic.make_priors(50)
    model = MG.build_product_model(MG.product_cfg(spec["overrides"]), priors, spec["seed"], device="cpu")     # same seed => same replica
    batch = synthetic.make_batch(1, 64, 64, num_gt=3, seed=50 + rank, priors=priors)                         # a different shard per rank
    A = 3 * sum((64 // s) ** 2 for s in (4, 8, 16, 32, 64))
    g = torch.Generator().manual_seed(900 + rank)
    model.proposal_generator.injected = {"E": torch.empty(1, A).exponential_(generator=g)}
    model.roi_heads.injected = {"E": torch.empty(1, 2048).exponential_(generator=g)}
    model.train()
    return model, batch


def _real_step(model, opt, batch, guard, staged):
    from omni3d_amd.cubercnn.solver.graphed import GraphedPipelined
    if staged:
        stepper = GraphedPipelined(model, opt, batch, model.prepack(batch), graphs=False)
        losses, _, pending = stepper()
        opt.all_reduce_finish(pending, defer_scale=True)
    else:
        opt.zero_grad()
        losses = model(batch)
        sum(losses.values()).backward()
        opt.all_reduce_grads()
    opt.check_nonfinite(guard.nonfinite_flag)
    skipped, retry, red = guard.update(losses)
    opt.step()
    return skipped, retry, red


def _worker_real(rank, world, port, out, staged):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _install_emulator()
    from oracle import make_golden as MG
    from omni3d_amd.cubercnn.solver import StepGuard, build_optimizer
    model, batch = _tiny_model_and_batch(rank)
    opt = build_optimizer(MG.product_cfg(MG.TINY["overrides"]), model)
    guard = StepGuard(["BoxHead/loss_cls", "BoxHead/loss_box_reg", "Cube/uncert", "Cube/loss_dims", "Cube/loss_xy", "Cube/loss_z",
                       "Cube/loss_pose", "Cube/loss_joint", "rpn/cls", "rpn/loc"], 0.01, 100, "cpu")
    opt.skip_flag = guard.skip
    skipped, retry, red = _real_step(model, opt, batch, guard, staged)
    torch.save({"param": opt.flat_param.clone(), "red": red, "skipped": skipped,
                "bn": model.backbone.bottom_up.level2.tree1.bn1.running_mean.clone()}, os.path.join(out, f"real{int(staged)}_{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.skipif(os.environ.get("OMNI_SLOW") != "1", reason="~20 min under the host emulator (four emulated model steps); set OMNI_SLOW=1")
def test_real_model_data_parallel_step_world2(emu_lib, tmp_path):
    """SURVEY.md 8(e) on the REAL model: two ranks, one image each, gradients all-reduced over gloo (the staged step's overlapped
    exchange and the single-phase one), divergence guard with its one collective, 1/world folded into the SGD kernel.  Replicas stay bit-identical,
    both exchange forms agree, per-rank BatchNorm statistics stay per-rank, and the result equals a single process that
    averages the two shards' gradients by hand."""
    world = 2
    for staged in (True, False):
        mp.spawn(_worker_real, args=(world, _free_port(), str(tmp_path), staged), nprocs=world, join=True)
    tp = [torch.load(os.path.join(tmp_path, f"real1_{r}.pt"), weights_only=False) for r in range(world)]
    sp = [torch.load(os.path.join(tmp_path, f"real0_{r}.pt"), weights_only=False) for r in range(world)]
    assert torch.equal(tp[0]["param"], tp[1]["param"]) and torch.equal(sp[0]["param"], sp[1]["param"])      # identical replicas
    assert (tp[0]["param"] - sp[0]["param"]).abs().max() <= 1e-6                                          # staged == single-phase
    assert tp[0]["red"] == tp[1]["red"] and not tp[0]["skipped"]                                          # same reduced losses everywhere
    assert not torch.equal(tp[0]["bn"], tp[1]["bn"])                                                      # BN running stats are per rank
    # single process, two replicas, hand-averaged gradients
    from oracle import make_golden as MG
    from omni3d_amd.cubercnn.solver import build_optimizer
    reps = [_tiny_model_and_batch(r) for r in range(world)]
    opts = [build_optimizer(MG.product_cfg(MG.TINY["overrides"]), m) for m, _ in reps]
    for (m, b), o in zip(reps, opts):
        o.zero_grad()
        sum(m(b).values()).backward()
    avg = (opts[0].flat_grad + opts[1].flat_grad) / world
    opts[0].flat_grad.copy_(avg)
    opts[0].step()
    assert (tp[0]["param"] - opts[0].flat_param).abs().max() <= 2e-6


# ---- the training script's own DistributedDataParallel wrapper (tools/train_net.py:449-454) around the product model -------------
LIGHT = ["MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", 16, "MODEL.RPN.BATCH_SIZE_PER_IMAGE", 16, "MODEL.RPN.PRE_NMS_TOPK_TRAIN", 100,
         "MODEL.RPN.POST_NMS_TOPK_TRAIN", 30, "MODEL.DLA.TYPE", "dla46_c", "MODEL.FPN.OUT_CHANNELS", 32, "MODEL.ROI_BOX_HEAD.FC_DIM", 64,
         "MODEL.ROI_CUBE_HEAD.FC_DIM", 64, "SOLVER.BASE_LR", 0.0002]


def _worker_ddp(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _install_emulator()
    from torch.nn.parallel import DistributedDataParallel
    from oracle import make_golden as MG
    from omni3d_amd import synthetic
    from omni3d_amd.cubercnn.modeling.meta_arch import build_model
    from omni3d_amd.cubercnn.solver import build_optimizer
    import omni3d_amd.cubercnn.modeling.backbone, omni3d_amd.cubercnn.modeling.proposal_generator, omni3d_amd.cubercnn.modeling.roi_heads  # noqa: F401,E401
    priors = synthetic.make_priors(50)
    cfg = MG.product_cfg(LIGHT)
    torch.manual_seed(100 + rank)                            # DIFFERENT random init per rank: the initial broadcast must fix it
    model = build_model(cfg, priors)                         # world 2 => prepared for the wrapper (cubercnn/solver/ddp.py)
    assert model._omni_owns_exchange and "_omni_ddp_anchor" not in model.state_dict()
    model.train()
    wrapped = DistributedDataParallel(model, broadcast_buffers=False, find_unused_parameters=True)      # as the reference does
    opt = build_optimizer(cfg, wrapped)                      # do_train builds it from the WRAPPED model (tools/train_net.py:124)
    assert opt._direct and opt.exchange_in_step and model._omni_auto is not None
    model._omni_auto.warm = 1
    reduced = []
    orig = dist.all_reduce

    def counting(t, *a, **kw):
        reduced.append(t.numel())
        return orig(t, *a, **kw)
    dist.all_reduce = counting
    per_iter = []
    pool = [synthetic.make_batch(1, 64, 64, num_gt=3, seed=300 + 10 * rank + s, priors=priors) for s in range(2)]
    torch.manual_seed(7 + rank)
    for it in range(3):                                      # 1 eager iteration, then replayed ones
        reduced.clear()
        loss_dict = wrapped(pool[it % 2])
        losses = sum(loss_dict.values())
        opt.zero_grad()
        losses.backward()
        opt.step()
        per_iter.append(sum(reduced))
    dist.all_reduce = orig
    torch.save({"param": opt.flat_param.clone(), "per_iter": per_iter, "bucket": opt.flat_grad.numel(), "replays": model._omni_auto.replays,
                "keys": list(model.state_dict().keys())[:3]}, os.path.join(out, f"ddp_{rank}.pt"))
    dist.destroy_process_group()


def test_script_ddp_wrapper_leaves_the_exchange_to_the_flat_bucket_world2(emu_lib, tmp_path):
    """The reference wraps the model in torch's DistributedDataParallel and builds the optimizer from the wrapped model.  The product
    then (a) still accumulates gradients directly into the flat bucket, (b) exchanges that bucket EXACTLY once per iteration (round 2
    did it twice: DDP's reducer, then the optimizer's safety net), on eager and on replayed iterations alike, (c) starts from rank
    0's weights although the ranks were initialised differently (DDP's constructor broadcast, done by build_optimizer for the
    parameters DDP was told to ignore), and (d) keeps the replicas bit-identical while the ranks see different data."""
    world = 2
    mp.spawn(_worker_ddp, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r = [torch.load(os.path.join(tmp_path, f"ddp_{k}.pt"), weights_only=False) for k in range(world)]
    assert torch.equal(r[0]["param"], r[1]["param"])
    assert r[0]["replays"] == 2 and r[1]["replays"] == 2
    for k in range(world):
        assert r[k]["per_iter"] == [r[k]["bucket"]] * 3, (r[k]["per_iter"], r[k]["bucket"])      # one pass over the bucket per iteration


# ---- round 4: one exchange range per backward stage -----------------------------------------------------------------------------
def _make_staged_net():
    """bottom_up.l0 | cut "a" | bottom_up.l1 -> features | cut | heads: three backward stages (heads, l1, l0)"""
    from omni3d_amd.cubercnn.modeling.layers import BatchNorm2d, Conv2d, FlattenLinear, Linear

    class BottomUp(torch.nn.Module):
        stage_cut = None
        stage_cut_at = ("a",)

        def __init__(self):
            super().__init__()
            self.l0 = Conv2d(8, 16, 3, padding=1, bias=True)
            self.bn0 = BatchNorm2d(16)
            self.l1 = Conv2d(16, 16, 3, padding=1, bias=True)

        def backward_stages(self):
            return {"l0": 2, "bn0": 2, "l1": 1}

        def forward(self, x):
            x = self.bn0(self.l0(x, relu=True), relu=True)
            if self.stage_cut is not None and self.training and torch.is_grad_enabled():
                x = self.stage_cut(x)
            return self.l1(x, relu=True)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.backbone = torch.nn.Module()
            self.backbone.bottom_up = BottomUp()
            self.f = FlattenLinear(16, 4, 12)
            self.l = Linear(12, 8)
            self.feature_cut = None

        def forward(self, x, packed=None):
            feats = {"p": self.backbone.bottom_up(x)}
            if self.feature_cut is not None:
                feats = self.feature_cut(feats)
            return {"loss": self.l(self.f(feats["p"], relu=True)).square().mean()}
    torch.manual_seed(0)
    return Net()


def _staged_opt(net):
    from omni3d_amd.cubercnn.solver.build import FlatSGD, grad_stage_map
    stage_of = grad_stage_map(net)
    for n, p in net.named_parameters():
        p._omni_grad_stage = stage_of(n)
    opt = FlatSGD([{"params": [p], "weight_decay": 0.0 if p.dim() == 1 else 1e-3} for p in net.parameters()], lr=0.1, momentum=0.9)
    opt.stage_cut_signature = tuple(net.backbone.bottom_up.stage_cut_at)
    return opt


def _worker_staged(rank, world, port, out, mixed):
    """mixed: rank 0 runs the staged step (an exchange behind every backward stage), rank 1 the plain loop whose step() exchanges the
    whole bucket -- what a rank whose capture failed does (solver/autoreplay.py).  Same collective sequence, same weights.
    mixed == 2: the same with the round-5 knobs (OMNI_EXCHANGE_MERGE_FROM / OMNI_EXCHANGE_CHUNK_MB): stages >= 1 go out together behind
    the last stage, in 4 KB pieces -- still one sequence on both ranks."""
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _install_emulator()
    from omni3d_amd.cubercnn.solver.graphed import GraphedPipelined
    net = _make_staged_net()
    opt = _staged_opt(net)
    if mixed == 2:
        type(opt).EXCHANGE_MERGE_FROM, type(opt).EXCHANGE_CHUNK = 1, 1024
        assert opt.exchange_stages(0) == [0] and opt.exchange_stages(1) == [] and opt.exchange_stages(2) == [1, 2]
    assert opt.n_stages == 3 and sorted(opt.stage_ranges) == [0, 1, 2]
    calls = []
    real = dist.all_reduce

    def counting(t, *a, **kw):
        calls.append(int(t.numel()))
        return real(t, *a, **kw)
    dist.all_reduce = counting
    staged = (rank == 0) or not mixed
    stepper = GraphedPipelined(net, opt, _shard(rank), None, graphs=False) if staged else None
    if stepper is not None:
        assert stepper._per_stage_exchange(3)
    for _ in range(2):
        if staged:
            _, _, pending = stepper()
            opt.all_reduce_finish(pending)
        else:
            opt.zero_grad()
            net(_shard(rank))["loss"].backward()
            opt.all_reduce_grads()
        opt.step()
    dist.all_reduce = real
    torch.save({"p": {n: p.detach().clone() for n, p in net.named_parameters()}, "calls": calls}, os.path.join(out, f"st{int(mixed)}{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.parametrize("mixed", [False, True, 2])
def test_per_stage_exchange_world2(emu_lib, tmp_path, mixed):
    """three backward stages, one exchange per stage behind its backward: replicas bit-identical, equal to the plain loop, and the
    sequence of all-reduce calls (sizes, order) is the same on a rank that runs the staged step and on one that does not"""
    world = 2
    mp.spawn(_worker_staged, args=(world, _free_port(), str(tmp_path), mixed), nprocs=world, join=True)
    r = [torch.load(os.path.join(tmp_path, f"st{int(mixed)}{k}.pt")) for k in range(world)]
    assert r[0]["calls"] == r[1]["calls"] and len(r[0]["calls"]) > 0
    if mixed == 2:
        assert max(r[0]["calls"]) <= 1024          # the chunk knob is honoured
    for n in r[0]["p"]:
        assert torch.equal(r[0]["p"][n], r[1]["p"][n]), n
    if not mixed:
        mp.spawn(_worker_single_phase_staged, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
        sp = torch.load(os.path.join(tmp_path, "sps0.pt"))
        for n in sp:
            assert (r[0]["p"][n] - sp[n]).abs().max() <= 1e-6 * max(1.0, float(sp[n].abs().max())), n


def _worker_single_phase_staged(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _install_emulator()
    net = _make_staged_net()
    opt = _staged_opt(net)
    for _ in range(2):
        opt.zero_grad()
        net(_shard(rank))["loss"].backward()
        opt.all_reduce_grads()
        opt.step()
    torch.save({n: p.detach().clone() for n, p in net.named_parameters()}, os.path.join(out, f"sps{rank}.pt"))
    dist.destroy_process_group()


def test_stage_ranges_of_the_real_model():
    """cubercnn_DLA34_FPN: seven backward stages (FC heads | ROIAlign + RPN | FPN + level 5, 4 | level 3 | level 2 | level 1, 0 | first layer);
    the ranges tile the bucket exactly once, every parameter sits in a range of its own stage, chunks are at most 32 MB, and what is
    left for after the last stage is the first layer's few kB (the backbone's 75 MB used to go out after the last stage)"""
    from oracle import make_golden as MG
    from omni3d_amd import synthetic
    from omni3d_amd.cubercnn.solver import build_optimizer
    cfg = MG.product_cfg([])
    model = MG.build_product_model(cfg, synthetic.make_priors(50), 3, device="cpu")
    opt = build_optimizer(cfg, model)
    assert opt.n_stages == 7 and opt.stage_cut_signature == ("stem", "l1", "p2", "p3", "pool")
    covered = sorted(r for rs in opt.stage_ranges.values() for r in rs)
    assert covered[0][0] == 0 and covered[-1][1] == opt.flat_grad.numel()
    assert all(a[1] == b[0] for a, b in zip(covered, covered[1:]))
    want = (("backbone.bottom_up.base_layer", 6), ("backbone.bottom_up.level0", 5), ("backbone.bottom_up.level1", 5),
            ("backbone.bottom_up.level2", 4), ("backbone.bottom_up.level3", 3), ("backbone.fpn_", 2),
            ("backbone.bottom_up.level5", 2), ("backbone.bottom_up.level4", 2), ("proposal_generator", 1), ("roi_heads", 0))
    for n, p in model.named_parameters():
        if id(p) not in opt._slot:
            continue
        off, cnt = opt._slot[id(p)]
        st = p._omni_grad_stage
        assert any(s <= off and off + cnt <= e for s, e in opt.stage_ranges[st]), (n, st)
        for prefix, stage in want:
            if n.startswith(prefix):
                assert st == stage, (n, st, stage)
    chunks = opt.exchange_chunks(range(opt.n_stages))
    assert max(e - s for s, e in chunks) <= opt.EXCHANGE_CHUNK and sum(e - s for s, e in chunks) == opt.flat_grad.numel()
    last = sum(e - s for s, e in opt.stage_ranges[6]) * 4
    assert last < 10 * 2 ** 20, last                       # bytes whose exchange cannot overlap any backward work
    by_stage = {k: sum(e - s for s, e in v) * 4 / 2 ** 20 for k, v in opt.stage_ranges.items()}
    assert by_stage[0] > 100 and by_stage[2] > 40, by_stage   # MB: FC heads 109, FPN + level 5 / 4 66


def test_exchange_tail_is_one_sequence_and_forms_agree():
    """the tiny ranges of the last backward stages (DLA-34: 0.5 / 0.03 / 0.01 MB) leave as ONE call sequence behind
    the last stage (default OMNI_EXCHANGE_MERGE_FROM=auto), touching ranges as one call -- and the sequence of (start, end) calls is the
    same whether a rank issues it stage by stage (staged replay) or as "early" + "late" (an eager step)."""
    import os
    os.environ.setdefault("OMNI_BENCH_DEVICE", "cpu")
    from omni3d_amd import bench_train as BT
    cfg, model, opt, _ = BT.build(1, device="cpu")
    assert opt.n_stages == 7
    mb = {k: 4 * sum(e - s for s, e in v) / 1e6 for k, v in opt.stage_ranges.items()}
    m = opt.merge_from()
    assert m == 4 and sum(mb[k] for k in range(m, 7)) < 2.0 and mb[3] > 2.0, (m, mb)
    per_stage = [c for k in range(7) for c in opt.exchange_chunks(opt.exchange_stages(k))]
    two_phase = opt.exchange_chunks([0]) + opt.exchange_chunks(list(range(1, 7)))
    assert per_stage == two_phase
    tail = opt.exchange_chunks(list(range(m, 7)))
    assert len(tail) <= 2 and sum(e - s for s, e in tail) == sum(e - s for k in range(m, 7) for s, e in opt.stage_ranges[k])      # one call per weight-decay class
    assert opt.exchange_stages(4) == [] and opt.exchange_stages(5) == [] and opt.exchange_stages(6) == [4, 5, 6]
    covered = sorted(per_stage)
    assert covered[0][0] == 0 and all(a[1] == b[0] for a, b in zip(covered, covered[1:])) and covered[-1][1] == opt.flat_grad.numel()
    # the round-4/5 behaviour stays reachable
    type(opt).EXCHANGE_MERGE_FROM = -1
    try:
        assert opt.merge_from() == -1 and opt.exchange_stages(5) == [5]
    finally:
        type(opt).EXCHANGE_MERGE_FROM = -2
