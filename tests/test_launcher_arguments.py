"""The argument checks of the evaluation launchers, characterised: for each launcher one smallest valid call, every tensor argument
broken in one way at a time (ValueError that names the argument, nothing launched), and the exact `L.call` sequence of the valid call.
Runs on the emulated library with CPU tensors.

A defect is a name of DEFECTS, or (name, pattern) where the message names another argument than the broken one: a launcher reads its
sizes from some arguments (K from cat_off, P from aff, I from dt_off, ...), so the wrong length of such an argument shows as the
mismatch of the next argument that has to agree with it.  A tensor on another device is reported as "one device" by the launchers that
compare devices and with the argument's name by `kitti`; the arguments a launcher reads back before it compares devices (the offsets
of `error_types`, `match_errors` and `box_annotate`, the bootstrap `weights`) and those of `det`, which leaves the device to
`lib.check_device`, have no such case.
"""
import inspect

import numpy as np
import pytest
import torch

from omni3d_amd import boxgen
from omni3d_amd import lib as omni_lib

I32, I64, U8, F32, F64 = torch.int32, torch.int64, torch.uint8, torch.float32, torch.float64
_OTHER = {I32: I64, I64: I32, U8: I32, F32: F64, F64: F32}


def _set(t, i, v):
    t = t.clone()
    t[i] = v
    return t


def _strided(t):
    """the right shape and values, every stride doubled"""
    return t.repeat_interleave(2, dim=-1)[..., ::2]


def _member(k, change):
    """apply `change` to member k of a tuple argument"""
    return lambda fit: tuple(change(t) if j == k % len(fit) else t for j, t in enumerate(fit))


DEFECTS = {
    "dtype": lambda t: t.to(_OTHER[t.dtype]),
    "float": lambda t: t.to(F32),                                   # for the index lists, which may be int32 or int64
    "length": lambda t: t[:-1],
    "ndim": lambda t: t.unsqueeze(0),
    "strided": _strided,
    "device": lambda t: torch.empty(t.shape, dtype=t.dtype, device="meta"),
    "not a tensor": lambda t: t.tolist(),
    "two elements": lambda t: torch.cat([t, t]),
    "start": lambda t: _set(t, 0, 1),                               # offsets that do not start at 0
    "decreasing": lambda t: _set(t, 1, int(t[-1]) + 1),             # ... that decrease (after rising past the total)
    "end": lambda t: _set(t, -1, int(t[-1]) - 1),                   # ... that do not end at the total
    "above": lambda t: _set(t, 0, 6),                               # an `order` entry that is no detection (sumD = 6)
    "below": lambda t: _set(t, 0, -1),
    "members": lambda fit: fit[:-1],
    "member dtype": _member(0, lambda t: t.to(_OTHER[t.dtype])),
    "member length": _member(0, lambda t: t[:-1]),
    "member strided": _member(0, _strided),
    "member device": _member(0, lambda t: torch.empty(t.shape, dtype=t.dtype, device="meta")),
    "last dtype": _member(-1, lambda t: t.to(_OTHER[t.dtype])),
    "last length": _member(-1, lambda t: t[:-1]),
}

DEV = ("device", "one device")
TENSOR = ["dtype", "length", "ndim", "strided", DEV]


# ---- the valid calls ---------------------------------------------------------------------------------------------------------------

def _boxes():
    return torch.from_numpy(boxgen.random_boxes(np.random.default_rng(0), 6))


def _merge():
    """2 categories x 3 detections, A = 2, T = 2, R = 3, M = 2"""
    g = torch.Generator().manual_seed(0)
    dt_match = torch.randint(-1, 1, (2, 2, 6), generator=g, dtype=I32)
    return dict(order=torch.arange(6, dtype=I32), cat_off=torch.tensor([0, 3, 6], dtype=I32), rank=torch.tensor([0, 1, 2, 0, 1, 2], dtype=I32),
                score=torch.linspace(0.9, 0.1, 6, dtype=F64), dt_match=dt_match, dt_ignore=torch.zeros((2, 2, 6), dtype=U8),
                npig=torch.full((2, 2), 2, dtype=I32), has_e=torch.ones(2, dtype=I32), rec_thrs=torch.tensor([0.0, 0.5, 1.0], dtype=F64),
                max_dets=torch.tensor([1, 3], dtype=I32), pair_row=torch.arange(6, dtype=I64), aff=torch.linspace(0.0, 1.0, 6, dtype=F64),
                lon=torch.linspace(-1.0, 1.0, 6, dtype=F64), err=torch.rand((6, 3), generator=g, dtype=F64),
                det_img=torch.tensor([0, 1, 0, 1, 0, 1], dtype=I32), weights=torch.tensor([[1, 1], [2, 0]], dtype=I32),
                npig_b=torch.full((2, 2, 2), 2, dtype=I32), has_e_b=torch.ones((2, 2), dtype=I32))


def _pick(d, names):
    return {k: d[k] for k in names.split()}


def _fit():
    from omni3d_amd.kernels import iou3d
    return iou3d.cuboid_fit(_boxes())


def _pairs(maker, a, b):
    i = torch.arange(6, dtype=I32)
    return lambda: {a: maker(), b: maker(), "idx1": i, "idx2": i.to(I64)}


def _footprints():
    from omni3d_amd.kernels import bev
    return bev.bev_footprints(_boxes())


def _rot(n):
    return torch.from_numpy(boxgen.rand_rot(np.random.default_rng(1), n).astype(np.float32)).contiguous()


def _intrinsics():
    return torch.tensor([[500.0, 0, 32, 0, 500, 24, 0, 0, 1]] * 2, dtype=F32)


def _match_errors():
    """two images, the second one empty: D = 3, G = 2"""
    g = torch.Generator().manual_seed(2)
    box = lambda n: torch.cat([torch.rand((n, 2), generator=g) * 10, torch.rand((n, 2), generator=g) * 10 + 5], 1)      # noqa: E731
    return dict(dt_box=box(3), dt_cat=torch.tensor([0, 1, 0], dtype=I32), dt_c2d=torch.rand((3, 2), generator=g), dt_z=torch.rand(3, generator=g) + 2,
                dt_dims=torch.rand((3, 3), generator=g) + 1, dt_pose=_rot(3), dt_off=torch.tensor([0, 3, 3], dtype=I32), gt_box=box(2),
                gt_cat=torch.tensor([0, 1], dtype=I32), gt_center=torch.rand((2, 3), generator=g) + 2, gt_dims=torch.rand((2, 3), generator=g) + 1,
                gt_pose=_rot(2).view(2, 9), gt_off=torch.tensor([0, 2, 2], dtype=I32), K=_intrinsics())


def _annotate():
    """two images, the second one empty: N = 3"""
    g = torch.Generator().manual_seed(3)
    box3d = torch.cat([torch.rand((3, 2), generator=g) - 0.5, torch.rand((3, 1), generator=g) + 4, torch.rand((3, 3), generator=g) + 0.5], 1)
    return dict(box3d=box3d, R=_rot(3), box_off=torch.tensor([0, 3, 3], dtype=I32), K=_intrinsics().view(2, 3, 3),
                size=torch.tensor([[64, 48], [64, 48]], dtype=I32))


def _error_types():
    """two images, the second one empty: sumD = 3, sumG = 2"""
    g = torch.Generator().manual_seed(4)
    return dict(sim=torch.rand(6, generator=g), dt_off=torch.tensor([0, 3, 3], dtype=I32), gt_off=torch.tensor([0, 2, 2], dtype=I32),
                dt_cat=torch.tensor([0, 1, 0], dtype=I32), dt_matched=torch.tensor([1, 0, 0], dtype=U8), dt_ignore=torch.zeros(3, dtype=U8),
                dt_score=torch.tensor([0.9, 0.8, 0.7], dtype=F64), gt_cat=torch.tensor([0, 1], dtype=I32), gt_matched=torch.tensor([1, 0], dtype=U8),
                gt_ignore=torch.zeros(2, dtype=U8), t_fg=0.5, t_bg=0.1)


def _slots():
    """B = 2 images of S = 3 slots"""
    return dict(verts=_boxes(), scores=torch.linspace(0.9, 0.4, 6), cls=torch.tensor([0, 1, 0, 1, 0, 1], dtype=I32), count=torch.tensor([3, 2], dtype=I32),
                iou_thr=0.5)


def _kitti_problem():
    """two images: 2 detections x 2 ground truths x 1 DontCare region, and an empty one; M = 1 metric"""
    return dict(dt_sizes=[2, 0], gt_sizes=[2, 0], dc_sizes=[1, 0], sim=torch.tensor([[0.8, 0.1, 0.2, 0.7]], dtype=F32), dc_ov=torch.zeros(2, dtype=F32),
                dt_code=torch.zeros(2, dtype=I32), dt_height=torch.full((2,), 40.0, dtype=F64), dt_score=torch.tensor([0.9, 0.8], dtype=F64),
                gt_code=torch.zeros(2, dtype=I32), gt_height=torch.full((2,), 40.0, dtype=F64), gt_occ=torch.zeros(2, dtype=I32),
                gt_trunc=torch.zeros(2, dtype=F64), cls_tab=[[0]], diffs=[[25.0, 2, 0.5]], min_ov=[[0.5]], dc_metric=[1])


def _kitti_aos(extra):
    def make():
        from omni3d_amd.kernels import kitti
        pb = kitti.Problem(**_kitti_problem())
        out = kitti.run_aos(pb, torch.zeros(2, dtype=F64), torch.zeros(2, dtype=F64), [1])
        every = dict(pb=pb, thr=out["thresholds"], K=out["K"], counts=out["counts"], sim_sum=out["sim_sum"], dt_alpha=torch.zeros(2, dtype=F64),
                     gt_alpha=torch.zeros(2, dtype=F64), aos_metric=[1])
        return _pick(every, extra)
    return make


MERGE = dict(order=["dtype", "ndim", "strided", DEV, "above", "below"],
             cat_off=["dtype", ("length", "cat_off|npig"), "ndim", "strided", DEV, "start", "decreasing", "end"],
             dt_match=["dtype", ("length", "dt_match|dt_ignore"), "ndim", "strided", DEV], dt_ignore=TENSOR, npig=TENSOR, has_e=TENSOR,
             rec_thrs=["dtype", "ndim", "strided", DEV])
RANKED = dict(MERGE, rank=TENSOR, max_dets=["dtype", "ndim", "strided", DEV])
PAIRS = dict(idx1=["float", "length", "ndim", DEV], idx2=["float", "length", "ndim", DEV])
FIT = ["members", "member dtype", "member length", "member strided", ("member device", "one device"), "last dtype", "last length"]
BOXES = ["dtype", "ndim", "strided", "not a tensor"]
BOXES_OF = [(d, "boxes") for d in BOXES]                       # the all-pairs forms hand each side to a launcher that calls it `boxes`
MATRICES = ["dtype", "length", "ndim", "strided", DEV]
KITTI_ROW = ["dtype", "length", "ndim", "device"]
SLOT_TABLE = dict(verts=["dtype", "length", "ndim"], scores=["dtype", "length", "ndim"], cls=["dtype", "length", "ndim"], count=["dtype", "ndim"])

# launcher -> (the valid call, the scalar arguments, argument -> its defects, the L.call sequence of the valid call: (entry, scalars))
LAUNCHERS = {
    "accumulate.accumulate": (
        lambda: _pick(_merge(), "order cat_off rank score dt_match dt_ignore npig has_e rec_thrs max_dets"), {"parallel", "block"},
        dict(RANKED, score=TENSOR),
        [("omni_eval_accumulate", (2, 2, 2, 2, 3, 6))]),
    "let.let_pairs": (
        _pairs(_fit, "fit1", "fit2"), {"tol_frac", "tol_min"}, dict(PAIRS, fit1=FIT, fit2=FIT),
        [("omni_let_pairs", (6, 6, 6, 0.1, 0.5))]),
    "let.box3d_let": (
        lambda: dict(boxes_dt=_boxes(), boxes_gt=_boxes()[:5]), {"tol_frac", "tol_min"}, dict(boxes_dt=BOXES_OF, boxes_gt=BOXES_OF),
        [("omni_cuboid_fit", (6, 1e-8, 1e-3)), ("omni_cuboid_fit", (5, 1e-8, 1e-3)), ("omni_let_pairs", (6, 5, 30, 0.1, 0.5))]),
    "let.accumulate_let": (
        lambda: _pick(_merge(), "order cat_off rank dt_match dt_ignore pair_row aff lon npig has_e rec_thrs max_dets"), set(),
        dict(RANKED, pair_row=TENSOR, aff=["dtype", ("length", "aff|lon"), "ndim", "strided", DEV], lon=TENSOR),
        [("omni_eval_accumulate_let", (6, 2, 2, 2, 2, 3, 6))]),
    "bootstrap.bootstrap_counts": (
        lambda: dict(grp_off=torch.tensor([0, 2, 4], dtype=I32), grp_img=torch.tensor([0, 1, 0, 1], dtype=I32), grp_npig=torch.full((4, 2), 1, dtype=I32),
                     weights=_merge()["weights"]), {"sum_gt"},
        dict(grp_off=["dtype", "length", "ndim", "strided", DEV, "start", "decreasing", "end"],
             grp_img=["dtype", ("length", "grp_img|grp_npig"), "ndim", "strided", DEV], grp_npig=TENSOR, weights=["dtype", "ndim", "strided"]),
        [("omni_eval_bootstrap_counts", (2, 2, 2, 4, 4, 2, 2))]),
    "bootstrap.bootstrap_accumulate": (
        lambda: _pick(_merge(), "order cat_off rank dt_match dt_ignore det_img weights npig_b has_e_b rec_thrs max_dets"), set(),
        dict({k: v for k, v in RANKED.items() if k not in ("npig", "has_e")}, det_img=TENSOR,
             cat_off=["dtype", ("length", "cat_off|npig_b"), "ndim", "strided", DEV, "start", "decreasing", "end"],
             weights=["dtype", ("length", "weights|npig_b"), "ndim", "strided"], npig_b=TENSOR, has_e_b=TENSOR),
        [("omni_eval_bootstrap", (2, 2, 2, 2, 2, 3, 6, 2, 2))]),
    "tperr.pair_errors": (
        _pairs(_fit, "fit1", "fit2"), {"up"}, dict(PAIRS, fit1=FIT, fit2=FIT),
        [("omni_pair_errors", (6, 6, 6, 0.0, 0.0, 0.0))]),
    "tperr.box3d_errors": (
        lambda: dict(boxes_dt=_boxes(), boxes_gt=_boxes()[:5]), {"up"}, dict(boxes_dt=BOXES_OF, boxes_gt=BOXES_OF),
        [("omni_cuboid_fit", (6, 1e-8, 1e-3)), ("omni_cuboid_fit", (5, 1e-8, 1e-3)), ("omni_pair_errors", (6, 5, 30, 0.0, 0.0, 0.0))]),
    "tperr.tp_errors": (
        lambda: dict(_pick(_merge(), "order cat_off dt_match dt_ignore pair_row err npig has_e rec_thrs"), dt_match=_merge()["dt_match"][:, 0].contiguous(),
                     dt_ignore=_merge()["dt_ignore"][:, 0].contiguous()), {"min_recall"},
        dict(MERGE, order=["dtype", "ndim", "strided", DEV], pair_row=TENSOR, err=["dtype", "ndim", "strided", DEV]),
        [("omni_eval_tp_errors", (6, 0.1, 2, 2, 3, 6))]),
    "errtypes.error_types": (
        _error_types, {"t_fg", "t_bg"},
        dict(sim=TENSOR, dt_off=["dtype", "length", "ndim", "strided", "start", "decreasing"],
             gt_off=["dtype", "length", "ndim", "strided", "start", "decreasing"], dt_cat=TENSOR, dt_matched=TENSOR, dt_ignore=TENSOR, dt_score=TENSOR,
             gt_cat=TENSOR, gt_matched=TENSOR, gt_ignore=TENSOR),
        [("omni_eval_error_types", (0.5, 0.1, 2, 3, 2, 2))]),
    "bev.bev_footprints": (
        lambda: dict(boxes=_boxes(), counts=torch.zeros(1, dtype=I32)), {"up", "eps_area"}, dict(boxes=BOXES, counts=["dtype", "two elements", "device"]),
        [("omni_bev_footprint", (6, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1e-8))]),
    "bev.bev_iou_pairs": (
        _pairs(_footprints, "fp1", "fp2"), set(), dict(PAIRS, fp1=FIT, fp2=FIT),
        [("omni_bev_iou_pairs", (6, 6, 6))]),
    "bev.bev_overlap": (
        lambda: dict(boxes_dt=_boxes(), boxes_gt=_boxes()[:5]), {"up", "eps_area"}, dict(boxes_dt=BOXES_OF, boxes_gt=BOXES_OF),
        [("omni_bev_footprint", (6, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1e-8)), ("omni_bev_footprint", (5, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1e-8)),
         ("omni_bev_iou_pairs", (6, 5, 30))]),
    "iou3d.cuboid_fit": (
        lambda: dict(boxes=_boxes(), counts=torch.zeros(1, dtype=I32)), {"eps_dim", "fit_tol"},
        dict(boxes=BOXES, counts=["dtype", "two elements", "device", "not a tensor"]),
        [("omni_cuboid_fit", (6, 1e-8, 1e-3))]),
    "iou3d.iou_fitted_pairs": (
        _pairs(_fit, "fit1", "fit2"), set(), dict(PAIRS, fit1=FIT, fit2=FIT),
        [("omni_iou3d_exact_pairs", (6, 6, 6))]),
    "iou3d.iou_box3d_exact": (
        lambda: dict(boxes1=_boxes(), boxes2=_boxes()[:5]), {"eps_dim", "fit_tol"}, dict(boxes1=BOXES_OF, boxes2=BOXES_OF),
        [("omni_cuboid_fit", (6, 1e-8, 1e-3)), ("omni_cuboid_fit", (5, 1e-8, 1e-3)), ("omni_iou3d_exact_pairs", (6, 5, 30))]),
    "viserr.match_errors": (
        _match_errors, set(),
        dict(dt_box=["dtype", ("length", "dt_box|dt_c2d"), "ndim", "strided", DEV], dt_cat=TENSOR, dt_c2d=TENSOR, dt_z=TENSOR, dt_dims=TENSOR, dt_pose=MATRICES,
             dt_off=["dtype", ("length", "dt_off|K"), "ndim", "strided", "start", "decreasing", "end"], gt_box=["dtype", ("length", "gt_box|gt_center"), "ndim", "strided", DEV], gt_cat=TENSOR, gt_center=TENSOR,
             gt_dims=TENSOR, gt_pose=MATRICES, gt_off=["dtype", "length", "ndim", "strided", "start", "decreasing", "end"], K=MATRICES),
        [("omni_match_errors", (2, 3, 2))]),
    "annotate.box_annotate": (
        _annotate, {"min_z"},
        dict(box3d=["dtype", ("length", "box3d|R"), "ndim", "strided", DEV], R=MATRICES, box_off=["dtype", ("length", "box_off|K"), "ndim", "strided", "start", "decreasing", "end"], K=MATRICES, size=TENSOR),
        [("omni_box_annotate", (2, 3, 0.2))]),
    "annotate.visibility_ragged": (
        _annotate, {"zplane"},
        dict(box3d=["dtype", ("length", "box3d|R"), "ndim", "strided", DEV], R=MATRICES, box_off=["dtype", ("length", "box_off|K"), "ndim", "strided", "start", "decreasing", "end"], K=MATRICES, size=TENSOR),
        [("omni_visibility_ragged", (2, 3, 24, 0.05))]),
    "kitti.box_params": (
        lambda: dict(corners=_boxes()), {"up"}, dict(corners=BOXES),
        [("omni_kitti_box_params", (6, 0.0, -1.0, 0.0))]),
    "kitti.Problem": (
        _kitti_problem, {"dt_sizes", "gt_sizes", "dc_sizes", "cls_tab", "diffs", "min_ov", "dc_metric"},
        dict(sim=["dtype", "length", "ndim"], dc_ov=KITTI_ROW, dt_code=KITTI_ROW, dt_height=KITTI_ROW, dt_score=KITTI_ROW, gt_code=KITTI_ROW,
             gt_height=KITTI_ROW, gt_occ=KITTI_ROW, gt_trunc=KITTI_ROW),
        []),
    "kitti.match_counts_aos": (
        _kitti_aos("pb thr K dt_alpha gt_alpha aos_metric"), {"pb", "thr", "K", "aos_metric", "out"}, dict(dt_alpha=KITTI_ROW, gt_alpha=KITTI_ROW),
        [("omni_kitti_match_counts_aos", (4, 1, 41, 2, 1, 1, 1, 1, 2, 2, 2, 2))]),
    "kitti.finalize_aos": (
        _kitti_aos("pb counts sim_sum K aos_metric"), {"pb", "counts", "K", "aos_metric", "out"}, dict(sim_sum=KITTI_ROW),
        [("omni_kitti_finalize_aos", (1, 1, 1, 41))]),
    "det.nms3d": (
        _slots, {"iou_thr", "class_agnostic", "eps_coplanar", "eps_nonzero", "method"}, SLOT_TABLE,
        [("omni_nms3d", (2, 3, 0.5, 1, 1e-4, 1e-8))]),
    "det.fuse3d": (
        lambda: dict(_slots(), aux=torch.rand((6, 2))), {"iou_thr", "views", "class_agnostic", "eps_coplanar", "eps_nonzero"},
        dict(SLOT_TABLE, verts=["dtype", "length", "ndim", "strided"], scores=["dtype", "length", "ndim", "strided"],
             cls=["dtype", "length", "ndim", "strided"], aux=["dtype", "length", "ndim", "strided"]),
        [("omni_fuse3d", (2, 3, 2, 1, 0.5, 0, 1e-4, 1e-8))]),
}


ALL_PAIRS = ("let.box3d_let", "tperr.box3d_errors", "bev.bev_overlap", "iou3d.iou_box3d_exact")


def _function(key):
    import importlib
    module, name = key.split(".")
    return getattr(importlib.import_module("omni3d_amd.kernels." + module), name)


def _record(monkeypatch, lib, forward=True):
    """wrap `lib.call`: -> the list of (entry, the arguments that are no pointers) of every call from now on"""
    calls, call = [], lib.call

    def wrapped(name, *args):
        calls.append((name, tuple(a for a, code in zip(args, omni_lib.SIGNATURES[name]) if code != "p")))
        if forward:
            call(name, *args)
    monkeypatch.setattr(lib, "call", wrapped)
    return calls


@pytest.mark.parametrize("key", sorted(LAUNCHERS))
def test_every_tensor_argument_has_a_rejection(key):
    _, scalars, table, _ = LAUNCHERS[key]
    assert all(table.values())
    assert set(table) | scalars == set(inspect.signature(_function(key)).parameters) and not set(table) & scalars


@pytest.mark.parametrize("key", sorted(LAUNCHERS))
def test_good_call_launches_what_it_did(key, emu_lib, monkeypatch):
    make, _, _, expected = LAUNCHERS[key]
    args = make()
    calls = _record(monkeypatch, emu_lib)
    _function(key)(**args)
    assert len(calls) == len(expected), calls
    for (name, scalars), (want_name, want) in zip(calls, expected):
        assert name == want_name and len(scalars) == len(want) and scalars == pytest.approx(want, rel=1e-15, abs=0), calls


@pytest.mark.parametrize("key", sorted(LAUNCHERS))
def test_rejections(key, emu_lib, monkeypatch):
    """one defect in one argument: ValueError that names the argument, and nothing is launched"""
    make, _, table, expected = LAUNCHERS[key]
    fn, good = _function(key), make()
    calls = _record(monkeypatch, emu_lib, forward=False)
    for name, defects in table.items():
        for defect in defects:
            defect, pattern = defect if isinstance(defect, tuple) else (defect, name)
            bad = DEFECTS[defect](good[name])
            with pytest.raises(ValueError, match=pattern):
                fn(**{**good, name: bad})
                pytest.fail(f"{key}: {name} with defect '{defect}' was accepted")
    # the all-pairs forms call one launcher per side, so the first side has been fitted when the second is refused; nothing else runs
    assert [c[0] for c in calls] == ([expected[0][0]] * len(table[list(table)[-1]]) if key in ALL_PAIRS else [])


def test_the_two_tightenings(emu_lib, monkeypatch):
    """`tp_errors` refuses an `order` that indexes outside the sumD detections, as the other three merge-order launchers do, and
    `bev_footprints` refuses a `counts` that is no tensor with ValueError, as `cuboid_fit` does"""
    from omni3d_amd.kernels import bev
    good = LAUNCHERS["tperr.tp_errors"][0]()
    calls = _record(monkeypatch, emu_lib, forward=False)
    for defect in ("above", "below"):
        with pytest.raises(ValueError, match="order"):
            _function("tperr.tp_errors")(**{**good, "order": DEFECTS[defect](good["order"])})
    with pytest.raises(ValueError, match="counts"):
        bev.bev_footprints(_boxes(), counts=[0])
    assert calls == []
