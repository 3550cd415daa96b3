"""Test-time augmentation for Cube R-CNN: `RCNN3DWithTTA(cfg, model)` runs every image at the sizes of TEST.AUG.MIN_SIZES and,
with TEST.AUG.FLIP, mirrored; brings the views' detections into one camera frame and one image resolution; and merges them with
ONE call of `kernels.det.fuse3d` (csrc/nms3d.hip, omni_fuse3d): cuboids whose exact IoU3D exceeds TEST.AUG.FUSE_IOU_THRESH become one
cuboid, the score-weighted mean of its members, whose score says how many of the views agreed.

detectron2 ships `GeneralizedRCNNWithTTA` for 2D boxes, merged by NMS; the reference has nothing for 3D.  Two things differ here.
A mirrored image shows the scene mirrored in X through a camera whose principal point is mirrored too (`mirror_K`), so what the model
says about it is brought back by `unmirror_detections`.  And cuboids cannot be averaged corner by corner: the same body may be
reported with its axes renamed, which the kernel resolves (include/omni3d_hip.h).

Whether this raises AP3D on real data has not been measured."""
import numpy as np
import torch
from torch import nn

from .... import functional as HF
from ....d2.structures import Boxes, Instances
from ....kernels import det, resize
from ...config.config import tta_args
from ..targets import pack_targets

# boxgen.UNIT / util.get_cuboid_verts_faces list the corners by the signs of their local (x, y, z): corner UNIT_FLIP_X[i] is corner i
# with the sign of x reversed
UNIT_FLIP_X = (1, 0, 3, 2, 5, 4, 7, 6)
MAX_SLOTS = det.NMS3D_MAX_SLOTS


def _const(like, values):
    if isinstance(like, torch.Tensor):
        return torch.tensor(values, dtype=like.dtype, device=like.device)
    return np.asarray(values, dtype=np.asarray(like).dtype)


def mirror_K(K, width):
    """the intrinsics of the horizontally flipped image of `width` pixels: pixel x goes to width - x, so does the principal point.
    The flipped image shows the scene mirrored in X through that camera.  -> a copy (a tensor for a tensor, else a float64 array)"""
    out = K.clone() if isinstance(K, torch.Tensor) else np.array(K, dtype=np.float64)
    out[0][2] = width - out[0][2]
    return out


def unmirror_detections(centre, pose, dims, verts, boxes=None, width=None):
    """3D outputs (and 2D boxes) of a mirrored view, back in the frame of the image as it was.  With M = diag(-1, 1, 1): the centre's
    X is negated; pose -> M pose M, a proper rotation again; the dimensions stay; the corners are negated in X and listed in the
    order that reverses the local x axis, which makes them the ordinary corner list of (centre, dims, pose); boxes (..., 4) are
    flipped as x -> width - x (width: a number or an array that broadcasts against boxes[..., 0]) with x1 and x2 swapped.
    Tensors or arrays with any leading dimensions -> (centre, pose, dims, verts, boxes)."""
    centre = centre * _const(centre, [-1.0, 1.0, 1.0])
    pose = pose * _const(pose, [[1.0, -1.0, -1.0], [-1.0, 1.0, 1.0], [-1.0, 1.0, 1.0]])
    verts = verts[..., list(UNIT_FLIP_X), :] * _const(verts, [-1.0, 1.0, 1.0])
    if boxes is not None:
        stack = torch.stack if isinstance(boxes, torch.Tensor) else np.stack
        boxes = stack([width - boxes[..., 2], boxes[..., 1], width - boxes[..., 0], boxes[..., 3]], -1)
    return centre, pose, dims, verts, boxes


def view_size(h, w, min_size, max_size):
    """detectron2's ResizeShortestEdge: the shorter side becomes min_size unless the longer one would then exceed max_size"""
    scale = min_size / min(h, w)
    nh, nw = (min_size, scale * w) if h < w else (scale * h, min_size)
    if max(nh, nw) > max_size:
        scale = max_size / max(nh, nw)
        nh, nw = nh * scale, nw * scale
    return int(nh + 0.5), int(nw + 0.5)


class RCNN3DWithTTA(nn.Module):
    """callable like the model in eval mode: wrapper(batched_inputs) -> [{"instances": Instances}] at the original resolution, with
    the fields of a plain inference pass, rows in descending score"""

    def __init__(self, cfg, model):
        super().__init__()
        if not hasattr(model, "_inference_device"):
            model = getattr(model, "module", model)                  # (a DistributedDataParallel wrapper)
        if not (hasattr(model, "_inference_device") and model._all_packed() and getattr(model.roi_heads, "replayable_inference", False)):
            raise TypeError("RCNN3DWithTTA needs an RCNN3D made of this package's proposal generator and ROI heads")
        a = tta_args(cfg)
        self.model = model
        self.max_size, self.thresh, self.class_agnostic = a["max_size"], a["fuse_iou_thresh"], a["class_agnostic"]
        self.views = [(s, f) for s in (a["min_sizes"] or (None,)) for f in ((False, True) if a["flip"] else (False,))]
        self.keep = int(cfg.TEST.DETECTIONS_PER_IMAGE)
        self.slots = int(model.roi_heads.box_predictor.test_topk_per_image)
        if len(self.views) * self.slots > MAX_SLOTS:
            raise ValueError(f"TEST.AUG: {len(self.views)} views x {self.slots} detections per view = {len(self.views) * self.slots} slots, "
                             f"the fusion kernel holds {MAX_SLOTS} per image")

    @property
    def device(self):
        return self.model.device

    def view_inputs(self, batched_inputs, min_size, flip):
        """the batch as one view sees it: images resized / mirrored on the device (the loader's `image` is the source, as in
        detectron2's TTA), `height` / `width` kept, the mirrored intrinsics for a flipped view"""
        out = []
        for info in batched_inputs:
            img = info["image"]
            h, w = img.shape[-2:]
            nh, nw = (h, w) if min_size is None else view_size(h, w, min_size, self.max_size)
            view = {k: v for k, v in info.items() if k not in ("image", "instances")}
            if flip or (nh, nw) != (h, w):
                img = resize.resize_bilinear_u8(img.to(self.device), nh, nw, flip=flip)
            view["image"] = img
            if flip:
                view["K"] = mirror_K(info["K"], info["width"])
            out.append(view)
        return out

    def infer_view(self, view_inputs):
        """the device half of one inference pass -> the tensors of `roi_heads_inference_device` on the fixed (B, topk) slots, no
        host synchronisation; replayed from the model's captured pass where it has one.  (Tests override this to plant detections.)"""
        model = self.model
        got = model._replayed_raw(view_inputs)
        if got is not None:
            return got[0]
        sizes = [(b["image"].shape[-2], b["image"].shape[-1]) for b in view_inputs]
        packed = pack_targets(view_inputs, sizes, getattr(model.roi_heads, "virtual_focal", 512.0), with_gt=False).to(model.device)
        with torch.no_grad(), HF.wino_weight_scope(model):
            return model._inference_device(view_inputs, packed)

    @torch.no_grad()
    def forward(self, batched_inputs):
        assert not self.model.training, "test-time augmentation runs a model in eval mode"
        if any("oracle2D" in b for b in batched_inputs):
            raise ValueError("test-time augmentation does not take oracle2D inputs: given 2D boxes are not detections to be merged")
        B, T = len(batched_inputs), len(self.views)
        HW = [(info["height"], info["width"]) for info in batched_inputs]
        per_view = []
        for min_size, flip in self.views:
            inputs = self.view_inputs(batched_inputs, min_size, flip)
            raw = self.infer_view(inputs)
            dev = raw["dbox"].device
            topk = raw["dbox"].shape[1]
            # 2D boxes at the original resolution: the products of `postprocess`, on the view's own size
            sc = torch.tensor([[W / b["image"].shape[-1], H / b["image"].shape[-2]] * 2 for (H, W), b in zip(HW, inputs)], dtype=torch.float32)
            dbox = raw["dbox"] * sc.to(dev, non_blocking=True)[:, None, :]
            cube3d = raw["cube3d"].view(B, topk, -1)
            centre, dims, c2d = cube3d[..., :3], cube3d[..., 3:6], cube3d[..., 6:8]
            pose, verts = raw["pose"].view(B, topk, 3, 3), raw["verts"].view(B, topk, 8, 3)
            if flip:
                width = torch.tensor([float(W) for _, W in HW], dtype=torch.float32).to(dev, non_blocking=True)[:, None]
                centre, pose, dims, verts, dbox = unmirror_detections(centre, pose, dims, verts, dbox, width)
                c2d = torch.stack([width - c2d[..., 0], c2d[..., 1]], -1)
            full = raw["full"].view(B, topk, -1)
            aux = torch.cat([dbox, full, centre, dims, pose.reshape(B, topk, 9), c2d], dim=2)
            used = torch.arange(topk, device=dev)[None, :] < raw["dcount"].view(B, 1)
            per_view.append((verts, raw["final"].view(B, topk), raw["dcls"].view(B, topk), aux, used))
        verts, score, cls, aux, used = (torch.cat(ts, dim=1) for ts in zip(*per_view))
        S, K = T * topk, aux.shape[2] - 21
        # the slots in use to the front, their order kept (a view's unused slots lie between those of the next)
        order = torch.argsort((~used).to(torch.int8), dim=1, stable=True)
        take = lambda t: torch.gather(t, 1, order.view(B, S, *([1] * (t.dim() - 2))).expand_as(t)).contiguous()       # noqa: E731
        verts, score, cls, aux = take(verts), take(score), take(cls), take(aux)
        count = used.sum(dim=1, dtype=torch.int32)
        f = det.fuse3d(verts.view(B * S, 8, 3), score.view(-1), cls.view(-1).int(), count, self.thresh, views=T, aux=aux.view(B * S, -1),
                       class_agnostic=self.class_agnostic)
        # a cluster of one is its detection as the model gave it; a fused one takes its parameters from the fused cuboid
        lone = (f.size == 1)[:, None]
        box, full = f.aux[:, :4], f.aux[:, 4:4 + K]
        centre = torch.where(lone, f.aux[:, 4 + K:7 + K], f.centre)
        dims = torch.where(lone, f.aux[:, 7 + K:10 + K], f.dims[:, [2, 1, 0]])                   # (w, h, l) lie along local (z, y, x)
        pose = torch.where(lone[:, :, None], f.aux[:, 10 + K:19 + K].reshape(-1, 3, 3), f.axes.transpose(1, 2))
        Ks = [np.asarray(info["K"].cpu() if isinstance(info["K"], torch.Tensor) else info["K"], dtype=np.float64) for info in batched_inputs]
        Kp = torch.tensor([[K[0][0], K[1][1], K[0][2], K[1][2]] for K in Ks], dtype=torch.float32).to(box.device, non_blocking=True)
        Kp = Kp.repeat_interleave(S, dim=0)
        z = torch.where(centre[:, 2] != 0, centre[:, 2], torch.ones_like(centre[:, 2]))
        proj = torch.stack([Kp[:, 0] * centre[:, 0] / z + Kp[:, 2], Kp[:, 1] * centre[:, 1] / z + Kp[:, 3]], dim=1)
        c2d = torch.where(lone, f.aux[:, 19 + K:21 + K], proj)
        counts = f.count.tolist()                                                                 # the one host sync
        results = []
        for n, (H, W) in enumerate(HW):
            k, o = min(counts[n], self.keep), n * S
            inst = Instances((H, W))
            inst.pred_boxes = Boxes(box[o:o + k])
            inst.scores = f.score[o:o + k]
            inst.scores_full = full[o:o + k]
            inst.pred_classes = f.cls[o:o + k].long()
            inst.pred_bbox3D = f.verts[o:o + k]
            inst.pred_center_cam = centre[o:o + k]
            inst.pred_center_2D = c2d[o:o + k]
            inst.pred_dimensions = dims[o:o + k]
            inst.pred_pose = pose[o:o + k]
            results.append(inst)
        from ..roi_heads.inference import postprocess
        return postprocess(results, batched_inputs, HW)                                           # clip, drop empty boxes
