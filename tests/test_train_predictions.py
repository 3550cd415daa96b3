"""`ROIHeads3D.want_predictions`: with the flag set the training branch returns, per image, the rows `RCNN3D.visualize_training`
draws -- picked by one launch of csrc/train_vis.hip -- with the fields of the reference's training-mode instances
(roi_heads.py:207-225, 771-822).  On the tiny synthetic model of tests/test_autoreplay.py:

  * every field equals `det.box_decode_gt_class` / `det.cube_decode` over the image's foreground prefix, gathered with the kernel's
    `keep_row`, bit for bit (the same kernels and device functions);
  * at most 20 rows per image;
  * the losses of the call are bit-identical to those of the same seeded call with the flag off."""
import pytest
import torch

from test_autoreplay import _build


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _forward(dev, want):
    """one seeded training forward of a fresh tiny model -> (loss dict, returned instances, what train_vis_pick saw and gave, model, batch)"""
    from omni3d_amd.kernels import det
    model, _, pool = _build(dev, images=2)
    model.__dict__["_omni_auto"] = None                      # plain eager launches
    heads = model.roi_heads
    got = {}
    inner = heads.forward

    def forward(*a, **k):
        out = inner(*a, **k)
        got["instances"] = out[0]
        return out

    heads.forward = forward
    pick = det.train_vis_pick

    def spy(pred, head, uncert_off, rois, cls, nfg, K, *a, **k):
        out = pick(pred, head, uncert_off, rois, cls, nfg, K, *a, **k)
        got["pick"] = dict(pred=pred, head=head, uncert_off=uncert_off, rois=rois, cls=cls, nfg=nfg, out=out)
        return out

    det.train_vis_pick = spy
    heads.want_predictions = want
    try:
        torch.manual_seed(0)
        losses = model(pool[0])
    finally:
        det.train_vis_pick = pick
        heads.want_predictions = False
    return {k: v.detach() for k, v in losses.items()}, got, model, pool[0]


def _run(dev):
    from omni3d_amd.kernels import det
    losses_off, got_off, _, _ = _forward(dev, False)
    assert got_off["instances"] == [] and "pick" not in got_off          # flag off: today's return value, no launch of the kernel
    losses_on, got, model, batch = _forward(dev, True)
    assert set(losses_on) == set(losses_off)
    for k in losses_on:
        assert torch.equal(_bits(losses_on[k]), _bits(losses_off[k])), k
    heads, inst, p = model.roi_heads, got["instances"], got["pick"]
    assert "_vis_pred" not in heads.__dict__ and "_vis_cube" not in heads.__dict__       # nothing outlives the call
    K, B = heads.num_classes, len(batch)
    S, Fc = heads.batch_size_per_image, p["cls"].shape[1]
    assert len(inst) == B and p["uncert_off"] == 12 * K
    keep_row, keep_count, keep_box, keep_score = p["out"]
    # the expected values: the existing launchers over the same tensors
    boxes = det.box_decode_gt_class(p["pred"], K, heads.last_sampled_classes.reshape(-1).contiguous(),
                                    heads.last_sampled_boxes.reshape(-1, 4).contiguous(), heads.box_predictor.box2box_weights).view(B, S, 4)
    packed = model.prepack(batch)
    priors = heads.priors_dims_per_cat.detach().reshape(K, 2, 3).contiguous()
    nfg, total = p["nfg"].tolist(), 0
    assert torch.equal(p["rois"], heads.last_sampled_boxes[:, :Fc]) and torch.equal(p["cls"], heads.last_sampled_classes[:, :Fc])
    for b in range(B):
        n, k, o = nfg[b], int(keep_count[b]), b * Fc
        total += k
        assert 0 <= k <= min(n, 20) and len(inst[b]) == k
        rows = keep_row[b, :k].long()
        assert (keep_row[b, k:] == -1).all() and (rows < n).all()
        img = torch.full((n,), b, dtype=torch.int32, device=p["head"].device)
        cube3d, pose, verts = det.cube_decode(p["head"][o:o + n].contiguous(), K, p["rois"][b, :n].contiguous(), p["cls"][b, :n].contiguous(), img,
                                              packed.Ks, packed.v2r, packed.ratio, priors, heads.cube_mode, heads.clusters())
        want = {"pred_boxes": boxes[b, :n][rows], "scores": keep_score[b, :k], "pred_classes": p["cls"][b, :n][rows].long(),
                "pred_center_cam": cube3d[rows, :3], "pred_dimensions": cube3d[rows, 3:6], "pred_pose": pose[rows],
                "pred_center_2D": cube3d[rows, 6:8], "pred_bbox3D": verts[rows]}
        assert set(inst[b].get_fields()) == set(want)
        for name, w in want.items():
            g = inst[b].get(name)
            g = g.tensor if name == "pred_boxes" else g
            assert g.shape == w.shape and g.dtype == w.dtype, name
            assert torch.equal(g.cpu(), w.cpu()) if g.dtype == torch.int64 else torch.equal(_bits(g), _bits(w)), name
        assert inst[b].pred_bbox3D.shape == (k, 8, 3) and inst[b].pred_pose.shape == (k, 3, 3)
        # the confidence the reference would sort by, exp(-uncertainty), is what cube_decode reports in its last column
        assert torch.allclose(keep_score[b, :k], cube3d[rows, 8], rtol=1e-6, atol=0)
    assert total > 0                                                     # the tiny model does sample foreground rows


def test_an_image_without_foreground_gives_empty_fields(emu_lib):
    """`_train_predictions` on hand-made tensors: image 0 has no foreground row, image 1 has two"""
    model, _, pool = _build("cpu", images=2)
    heads = model.roi_heads
    K, S, Fc = heads.num_classes, heads.batch_size_per_image, heads.fg_cap
    g = torch.Generator().manual_seed(3)
    ldh = 13 * K
    heads.__dict__["_vis_pred"] = torch.randn(2 * S, 5 * K + 1, generator=g)
    rois = torch.tensor([[10.0, 10.0, 40.0, 50.0], [30.0, 20.0, 60.0, 60.0]]).repeat(Fc, 1)[:2 * Fc].contiguous()
    cls = torch.randint(K, (2 * Fc,), generator=g, dtype=torch.int32)
    bidx = torch.arange(2, dtype=torch.int32).repeat_interleave(Fc)
    heads.__dict__["_vis_cube"] = (torch.randn(2 * Fc, ldh, generator=g), rois, cls, bidx)
    counts = torch.tensor([[0, S], [2, S - 2]], dtype=torch.int32)
    out = heads._train_predictions([(64, 64), (64, 64)], rois.view(2, Fc, 4), counts, model.prepack(pool[0]))
    assert len(out[0]) == 0 and 1 <= len(out[1]) <= 2
    assert out[0].pred_boxes.tensor.shape == (0, 4) and out[0].pred_bbox3D.shape == (0, 8, 3) and out[0].pred_pose.shape == (0, 3, 3)
    assert out[0].pred_center_cam.shape == (0, 3) and out[0].scores.shape == (0,) and out[0].pred_classes.dtype == torch.int64


def test_want_predictions_emulated(emu_lib):
    _run("cpu")


@pytest.mark.gpu
def test_want_predictions_gpu(hip_lib):
    _run("cuda")
