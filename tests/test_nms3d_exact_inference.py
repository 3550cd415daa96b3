"""TEST.NMS_3D.IOU_TYPE "exact" through the inference path, on the synthetic model and batch of tests/test_nms3d_inference.py (imported
as a module: same seeds, so the feature-off pass is that module's):

 (i)   config: `add_nms3d_exact_config` adds IOU_TYPE (default "evaluator") to the three keys of `add_nms3d_config`, is idempotent,
       and `ROIHeads3D.from_config` picks the key up; without the call the node has exactly the three keys and the model decides as
       before; `demo.py --nms3d 0.25 --nms3d-iou exact` sets both;
 (ii)  calls: with "exact" the pass makes the library calls of the feature-off pass plus omni_nms3d_exact, once, and no omni_nms3d;
 (iii) results: the Instances are those of the feature off with the rows taken out that the float64 reference removes
       (test_nms3d_inference._reference_rows and its ambiguity rule), all nine fields, order kept;
 (iv)  replay: the signature's entry is ("nms3d", thr, agnostic, "exact"); a replayed pass equals the eager one; switching the type
       on a live InferReplay is another signature and another capture, never a stale replay, and the default's entry is the 3-tuple."""
import functools
import importlib.util
import os

import pytest
import torch

import test_nms3d_inference as T
from conftest import ROOT

THR = T.THR


def _cfg_exact():
    from oracle import make_golden as MG
    from omni3d_amd.cubercnn import config as C
    cfg = MG.product_cfg(T.LIGHT)
    C.add_nms3d_exact_config(cfg)
    cfg.merge_from_list(["TEST.NMS_3D.ENABLED", True, "TEST.NMS_3D.IOU_THRESH", THR, "TEST.NMS_3D.IOU_TYPE", "exact"])
    return cfg


@functools.lru_cache(maxsize=None)
def _model(dev):
    from oracle import make_golden as MG
    return MG.sharpen(MG.build_product_model(_cfg_exact(), T._priors(), T.MODEL_SEED, device="cpu")).to(dev).eval()


@functools.lru_cache(maxsize=None)
def _eager(dev):
    from omni3d_amd.cubercnn.modeling.meta_arch import infer_replay
    prev = infer_replay.ENABLED
    try:
        infer_replay.ENABLED = False
        return T._pass(_model(dev), T._batch(dev))
    finally:
        infer_replay.ENABLED = prev


def _calls_and_rows(dev):
    heads = _model(dev).roi_heads
    assert heads.nms3d_thresh == THR and heads.nms3d_class_agnostic is True and heads.nms3d_iou_type == "exact"
    calls_off, calls_on = T._eager(dev, "off")["calls"], _eager(dev)["calls"]
    assert calls_on.count("omni_nms3d_exact") == 1 and "omni_nms3d" not in calls_on
    assert [c for c in calls_on if c != "omni_nms3d_exact"] == calls_off                      # one call more, nothing else
    off, on = T._eager(dev, "off")["instances"], _eager(dev)["instances"]
    rows = []
    for inst in off:
        keep, ambiguous = T._reference_rows(inst, THR)
        rows.append(None if ambiguous else keep)
    skipped = sum(r is None for r in rows)
    assert skipped <= 1
    if dev == "cpu":
        assert skipped == 0
    assert sum(len(i) - len(r) for i, r in zip(off, rows) if r is not None) >= 1, "nothing to remove: the test shows nothing"
    T._same(off, on, rows)


def _replay(dev):
    from omni3d_amd.cubercnn.modeling.meta_arch import infer_replay
    model, batch = _model(dev), T._batch(dev)
    want = {"exact": _eager(dev)["instances"], "evaluator": T._eager(dev, THR)["instances"]}
    prev = infer_replay.ENABLED
    try:
        infer_replay.ENABLED = True
        rep = model.__dict__["_omni_infer"] = infer_replay.InferReplay(model, graphs=False if dev == "cpu" else None)
        sig = rep.signature(batch)
        assert sig[:3] == (2, 64, 64) and sig[3] == ("nms3d", THR, True, "exact")
        T._pass(model, batch)                                               # pass 1 of the bucket: eager
        got = [T._pass(model, batch)["instances"] for _ in range(2)]
        assert rep.failed is None and rep.captures == 1 and rep.replays == 2, (rep.failed, rep.captures, rep.replays)
        T._same(want["exact"], got[0]), T._same(want["exact"], got[1])
        model.roi_heads.nms3d_iou_type = "evaluator"                        # another type: another signature, another capture
        assert rep.signature(batch) != sig and rep.signature(batch)[3] == ("nms3d", THR, True)
        first = T._pass(model, batch)
        assert rep.replays == 2 and first["calls"].count("omni_nms3d") == 1 and "omni_nms3d_exact" not in first["calls"]
        second = T._pass(model, batch)["instances"]
        assert rep.failed is None and rep.captures == 2 and rep.replays == 3
        T._same(want["evaluator"], first["instances"]), T._same(want["evaluator"], second)
        model.roi_heads.nms3d_iou_type = "exact"
        back = T._pass(model, batch)["instances"]
        assert rep.captures == 2 and rep.replays == 4
        T._same(want["exact"], back)
    finally:
        infer_replay.ENABLED = prev
        model.roi_heads.nms3d_iou_type = "exact"
        model.__dict__.pop("_omni_infer", None)


def test_exact_calls_and_reference_rows_emulated(emu_lib):
    _calls_and_rows("cpu")


def test_exact_replay_follows_the_type_emulated(emu_lib):
    _replay("cpu")


@pytest.mark.gpu
def test_exact_calls_and_reference_rows_gpu(hip_lib):
    _calls_and_rows("cuda")


@pytest.mark.gpu
def test_exact_replay_follows_the_type_gpu(hip_lib):
    _replay("cuda")


def test_config_key_and_demo_switch(emu_lib, tmp_path):
    from omni3d_amd.cubercnn.config import add_nms3d_config, add_nms3d_exact_config
    from omni3d_amd.cubercnn.modeling.roi_heads.roi_heads import ROIHeads3D
    shape = T._model("cpu", "plain").backbone.output_shape()
    cfg = T._cfg("plain")
    add_nms3d_config(cfg)                                                    # without the new call: today's three keys, today's model
    assert dict(cfg.TEST.NMS_3D) == {"ENABLED": False, "IOU_THRESH": 0.25, "CLASS_AGNOSTIC": True}
    assert ROIHeads3D.from_config(cfg, shape)["nms3d_iou_type"] == "evaluator"
    assert T._model("cpu", THR).roi_heads.nms3d_iou_type == "evaluator"
    assert add_nms3d_exact_config(cfg) is cfg
    assert dict(cfg.TEST.NMS_3D) == {"ENABLED": False, "IOU_THRESH": 0.25, "CLASS_AGNOSTIC": True, "IOU_TYPE": "evaluator"}
    cfg.merge_from_list(["TEST.NMS_3D.IOU_TYPE", "exact", "TEST.NMS_3D.ENABLED", True, "TEST.NMS_3D.IOU_THRESH", 0.4])
    add_nms3d_exact_config(cfg)                                              # idempotent: the values that were set stay
    assert dict(cfg.TEST.NMS_3D) == {"ENABLED": True, "IOU_THRESH": 0.4, "CLASS_AGNOSTIC": True, "IOU_TYPE": "exact"}
    args = ROIHeads3D.from_config(cfg, shape)
    assert args["nms3d_thresh"] == 0.4 and args["nms3d_iou_type"] == "exact"
    fresh = T._cfg("plain")
    add_nms3d_exact_config(fresh)                                            # on a cfg without the node: it adds the node too
    assert dict(fresh.TEST.NMS_3D) == {"ENABLED": False, "IOU_THRESH": 0.25, "CLASS_AGNOSTIC": True, "IOU_TYPE": "evaluator"}
    cfg.merge_from_list(["TEST.NMS_3D.IOU_TYPE", "bev"])
    with pytest.raises(ValueError):
        ROIHeads3D(**ROIHeads3D.from_config(cfg, shape))
    # demo.py
    spec = importlib.util.spec_from_file_location("omni3d_demo_nms3d_exact", os.path.join(ROOT, "demo", "demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    common = ["--config-file", os.path.join(ROOT, "configs", "cubercnn_DLA34_FPN.yaml"), "--input-folder", str(tmp_path)]
    out = ["OUTPUT_DIR", str(tmp_path / "out")]
    cfg = demo.setup(demo.argument_parser().parse_args(common + ["--nms3d", "0.25", "--nms3d-iou", "exact"] + out))
    assert cfg.TEST.NMS_3D.ENABLED is True and cfg.TEST.NMS_3D.IOU_THRESH == 0.25 and cfg.TEST.NMS_3D.IOU_TYPE == "exact"
    cfg = demo.setup(demo.argument_parser().parse_args(common + ["--nms3d", "0.25"] + out))
    assert cfg.TEST.NMS_3D.ENABLED is True and cfg.TEST.NMS_3D.IOU_TYPE == "evaluator"
    with pytest.raises(SystemExit):
        demo.argument_parser().parse_args(common + ["--nms3d-iou", "bev"])
