"""The IoU regression losses inside the model: MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE giou with MODEL.RPN.OBJECTNESS_UNCERTAINTY none and
MODEL.RPN.BBOX_REG_LOSS_TYPE diou train through the drop-in loop, eagerly and from the captured step (the kernels make no host
synchronisation and no allocation of their own), and their gradients reach both regression layers."""
import math

import pytest
import torch

import test_autoreplay as T
from test_bn_frozen_model import SMALL, _close_logs

BOX_REG = ["MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE", "giou", "MODEL.RPN.OBJECTNESS_UNCERTAINTY", "none", "MODEL.RPN.BBOX_REG_LOSS_TYPE", "diou"]


def _check_log(model, log):
    """all losses finite; GIoU is bounded by 2 per foreground row, so loss_box_reg (sum over the foreground rows / all rows) lies in
    [0, 2 x foreground share]"""
    for entry in log:
        assert all(math.isfinite(v) for v in entry.values()), entry
        assert 0.0 <= entry["BoxHead/loss_box_reg"] <= 2.0 and entry["rpn/loc"] >= 0.0, entry
    s = model.roi_heads.box_predictor.pending_logs["fast_rcnn"].tolist()             # the sums of the last step
    assert s[3] > 0 and 0.0 < log[-1]["BoxHead/loss_box_reg"] <= 2.0 * s[3] / max(s[2], 1.0) * (1 + 1e-6), (s, log[-1])


@pytest.mark.gpu
def test_iou_losses_loop_replay_gpu(hip_lib):
    """captured and replayed steps with the IoU losses in both stages log the losses of eager launches (the tolerances of
    test_bn_frozen_model.py::test_frozen_bn_dropin_loop_replay_gpu for the L1 model)"""
    runs = []
    for replay in (True, False):
        model, opt, pool = T._build("cuda", SMALL + BOX_REG, 128)
        assert model.roi_heads.box_predictor.box_reg_loss_type == "giou" and model.proposal_generator.box_reg_loss_type == "diou"
        if not replay:
            model.__dict__["_omni_auto"] = None
        else:
            model._omni_auto.warm = 1
        log = T._loop(model, opt, pool, 4)
        _check_log(model, log)
        runs.append((model, log))
    (ma, la), (mb, lb) = runs
    auto = ma._omni_auto
    assert auto.failed is None and auto.replays == 3, (auto.failed, auto.replays)
    _close_logs(la, lb, 1e-3)


def test_iou_losses_train_step_emulated(emu_lib):
    """one training step of the same losses on the host-compiled kernels (the light model of test_autoreplay.py, as the other emulated
    loop tests use: the emulator is slow on a 128 px DLA-34 step): finite, bounded losses, and nonzero finite gradients in the regression layers of both stages"""
    model, opt, pool = T._build("cpu", T.LIGHT + BOX_REG, 64)
    model.__dict__["_omni_auto"] = None
    torch.manual_seed(0)
    loss_dict = model(pool[0])
    _check_log(model, [{k: float(v.detach()) for k, v in loss_dict.items()}])
    opt.zero_grad()
    sum(loss_dict.values()).backward()
    for w in (model.roi_heads.box_predictor.bbox_pred.weight, model.proposal_generator.rpn_head.anchor_deltas.weight):
        assert w.grad is not None and bool(torch.isfinite(w.grad).all()) and bool(w.grad.abs().max() > 0)
