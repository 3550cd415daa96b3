"""The view algebra of test-time augmentation (cubercnn/modeling/meta_arch/tta.py), no network involved.

`mirror_K` / `unmirror_detections`, float64 numpy: a random scene of cuboids is projected through K; the scene mirrored in X is
projected through mirror_K(K, W); the pixels must be the horizontal flip (x -> W - x) of the first projection.  The mirrored cuboids,
written as a model looking at the mirrored scene would write them (centre M c, the proper rotation M R M, the corners of those in
the ordinary order), come back through `unmirror_detections` as the originals: corners in `UNIT` order and equal to the corners
regenerated from the returned centre / dimensions / pose, pose with det +1, 2D boxes flipped back.  Float64 throughout: 1e-12.

`RCNN3DWithTTA` with planted detections: the per-view method is overridden to return three views of three objects -- one view
mirrored and expressed in the mirrored frame on a mirrored image, one at another resolution and missing an object -- and the
wrapper's Instances must equal the numpy fusion (tests/test_fuse3d.py::fuse64) of the planted boxes brought back by hand: 3D fields
within the tolerances of tests/test_fuse3d.py (coordinates below 64), 2D boxes, centre projections and class scores within 1e-4
(a handful of float32 operations on values below 100: 6e-6 each).  The object seen in 2 of 3 views carries (s1 + s2) / 3."""
import numpy as np
import pytest
import torch

from omni3d_amd import boxgen
from test_fuse3d import POS_TOL, REL_TOL, fuse64
from test_iou3d_exact import _axis_turn, fit64

W_IMG, H_IMG = 96, 64
K_IMG = [[70.0, 0.0, 50.0], [0.0, 72.0, 30.0], [0.0, 0.0, 1.0]]
M = np.diag([-1.0, 1.0, 1.0])
PIX_TOL = 1e-4


def _corners64(c, d_lhw, R):
    return c[:, None, :] + np.einsum("nij,nkj->nki", R, boxgen.UNIT[None] * d_lhw[:, None, :])


def _project(p, K):
    K = np.asarray(K, np.float64)
    return np.stack([K[0, 0] * p[..., 0] / p[..., 2] + K[0, 2], K[1, 1] * p[..., 1] / p[..., 2] + K[1, 2]], -1)


def test_mirror_and_unmirror_are_the_flip_of_the_scene():
    from omni3d_amd.cubercnn.modeling.meta_arch import tta
    rng = np.random.default_rng(3)
    n = 40
    c = np.stack([rng.uniform(-8, 8, n), rng.uniform(-2, 2, n), rng.uniform(4, 40, n)], 1)
    d, R = rng.uniform(0.4, 4.0, size=(n, 3)), boxgen.rand_rot(rng, n)
    verts = _corners64(c, d, R)
    Km = tta.mirror_K(K_IMG, W_IMG)
    assert isinstance(Km, np.ndarray) and Km[0, 2] == W_IMG - K_IMG[0][2] and K_IMG[0][2] == 50.0           # a copy
    assert np.array_equal(np.delete(Km.ravel(), 2), np.delete(np.asarray(K_IMG).ravel(), 2))
    Kt = tta.mirror_K(torch.tensor(K_IMG), W_IMG)
    assert isinstance(Kt, torch.Tensor) and float(Kt[0, 2]) == W_IMG - 50.0
    # the mirrored scene through the mirrored camera is the flipped image
    pix, pix_m = _project(verts, K_IMG), _project(verts @ M, Km)
    assert np.abs(pix_m[..., 0] - (W_IMG - pix[..., 0])).max() <= 1e-12 and np.abs(pix_m[..., 1] - pix[..., 1]).max() <= 1e-12
    # what a model looking at the mirrored scene reports: the mirrored body with a PROPER pose, corners in the ordinary order
    c_m, R_m = c @ M, M @ R @ M
    verts_m = _corners64(c_m, d, R_m)
    for k in range(n):                                                                                       # the same body as the mirrored one
        a, b = verts_m[k], verts[k] @ M
        assert np.abs(a[:, None, :] - b[None, :, :]).max(2).min(1).max() <= 1e-12
    assert np.abs(verts_m - verts @ M).max() > 0.1                                                          # but not corner for corner
    boxes = np.stack([pix[..., 0].min(1), pix[..., 1].min(1), pix[..., 0].max(1), pix[..., 1].max(1)], 1)
    boxes_m = np.stack([pix_m[..., 0].min(1), pix_m[..., 1].min(1), pix_m[..., 0].max(1), pix_m[..., 1].max(1)], 1)
    c2, R2, d2, v2, b2 = tta.unmirror_detections(c_m, R_m, d, verts_m, boxes_m, W_IMG)
    assert np.abs(c2 - c).max() <= 1e-12 and np.abs(R2 - R).max() <= 1e-12 and d2 is d and np.abs(b2 - boxes).max() <= 1e-12
    assert np.abs(np.linalg.det(R2) - 1.0).max() <= 1e-12 and np.abs(R2 @ R2.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-12
    assert np.abs(v2 - verts).max() <= 1e-12                                                                 # UNIT order again
    assert np.abs(v2 - _corners64(c2, d2, R2)).max() <= 1e-12
    assert (b2[:, 0] < b2[:, 2]).all()
    # applying it twice is the identity; tensors give what arrays give, with leading dimensions
    back = tta.unmirror_detections(c2, R2, d2, v2, b2, W_IMG)
    assert np.array_equal(back[0], c_m) and np.array_equal(back[1], R_m) and np.array_equal(back[3], verts_m) and np.abs(back[4] - boxes_m).max() <= 1e-12
    t = tta.unmirror_detections(torch.from_numpy(c_m).view(4, 10, 3), torch.from_numpy(R_m).view(4, 10, 3, 3), torch.from_numpy(d).view(4, 10, 3),
                                torch.from_numpy(verts_m).view(4, 10, 8, 3), torch.from_numpy(boxes_m).view(4, 10, 4),
                                torch.full((4, 1), float(W_IMG), dtype=torch.float64))
    for got, want in zip(t, (c2, R2, d2, v2, b2)):
        assert got.shape[:2] == (4, 10) and np.array_equal(got.reshape(want.shape).numpy(), want)
    assert tta.unmirror_detections(c_m, R_m, d, verts_m)[4] is None
    assert tta.view_size(480, 640, 600, 4000) == (600, 800) and tta.view_size(480, 640, 600, 700) == (525, 700) and tta.view_size(64, 48, 48, 100) == (64, 48)


class _Heads:
    replayable_inference = True

    class box_predictor:
        test_topk_per_image = 4


class _StubModel(torch.nn.Module):
    """what RCNN3DWithTTA asks of a model before the per-view method (overridden below) would run it"""
    roi_heads = _Heads()

    def __init__(self, dev):
        super().__init__()
        self._dev = torch.device(dev)

    device = property(lambda self: self._dev)

    def _all_packed(self):
        return True

    def _inference_device(self, batched_inputs, packed):
        raise AssertionError("the per-view method is overridden")


def _planted(dev):
    """three objects, three views (plain | mirrored | another size, object C missing) -> the raw view outputs a model would give, and
    the detections brought back into the frame and resolution of the image by hand, float64"""
    rng = np.random.default_rng(9)
    Kn, TOPK = 3, 4
    base_c = np.array([[-4.0, 0.5, 12.0], [3.0, -0.5, 20.0], [0.5, 1.0, 35.0]])
    base_d = rng.uniform(1.0, 3.0, size=(3, 3))                      # (l, h, w) along local (x, y, z)
    base_R = boxgen.rand_rot(rng, 3)
    views = [dict(size=(32, 48), flip=False, objects=(0, 1, 2)), dict(size=(32, 48), flip=True, objects=(2, 0, 1)),
             dict(size=(40, 60), flip=False, objects=(1, 0))]
    raws, seen = [], {0: [], 1: [], 2: []}
    for v in views:
        h, w = v["size"]
        raw = dict(dbox=np.tile(np.array([0.0, 0.0, 1.0, 1.0], np.float32), (1, TOPK, 1)), final=np.zeros(TOPK, np.float32),
                   full=np.zeros((1, TOPK, Kn), np.float32), dcls=np.zeros((1, TOPK), np.int32), verts=np.zeros((TOPK, 8, 3), np.float32),
                   cube3d=np.zeros((TOPK, 9), np.float32), pose=np.zeros((TOPK, 3, 3), np.float32), dcount=np.array([len(v["objects"])], np.int32))
        raw["final"][:] = 0.99                                        # behind the count: the best score of the view, never read
        for s, obj in enumerate(v["objects"]):
            c = base_c[obj] + rng.normal(scale=0.02, size=3) * base_d[obj]
            d = base_d[obj] * rng.uniform(0.97, 1.03, size=3)
            R = _axis_turn(rng.normal(size=3), np.radians(rng.uniform(0.0, 1.0))) @ base_R[obj]
            score, full = rng.uniform(0.3, 0.9), rng.dirichlet(np.ones(Kn))
            pix = _project(_corners64(c[None], d[None], R[None])[0], K_IMG)
            box = np.array([pix[:, 0].min(), pix[:, 1].min(), pix[:, 0].max(), pix[:, 1].max()])        # at the image's resolution
            c2d = _project(c, K_IMG)
            cm, Rm, boxm, c2dm = c, R, box, c2d
            if v["flip"]:                                             # as the mirrored view sees it
                cm, Rm = M @ c, M @ R @ M
                boxm = np.array([W_IMG - box[2], box[1], W_IMG - box[0], box[3]])
                c2dm = np.array([W_IMG - c2d[0], c2d[1]])
            raw["dbox"][0, s] = boxm / np.array([W_IMG / w, H_IMG / h] * 2)                             # at the view's resolution
            raw["final"][s], raw["full"][0, s], raw["dcls"][0, s] = score, full, obj
            raw["verts"][s] = _corners64(cm[None], d[None], Rm[None])[0]
            raw["cube3d"][s] = np.concatenate([cm, d[[2, 1, 0]], c2dm, [1.0]])
            raw["pose"][s] = Rm
            # back by hand, from the float32 values the wrapper is given
            v32 = raw["verts"][s].astype(np.float64)
            b32 = raw["dbox"][0, s].astype(np.float64) * np.array([W_IMG / w, H_IMG / h] * 2)
            if v["flip"]:
                v32 = (v32 * np.array([-1.0, 1.0, 1.0]))[[1, 0, 3, 2, 5, 4, 7, 6]]
                b32 = np.array([W_IMG - b32[2], b32[1], W_IMG - b32[0], b32[3]])
            seen[obj].append(dict(score=float(raw["final"][s]), verts=v32, box=b32, full=raw["full"][0, s].astype(np.float64)))
        raws.append({k: torch.from_numpy(a).to(dev) for k, a in raw.items()})
    want = []
    for obj, members in seen.items():
        members.sort(key=lambda m: -m["score"])                       # rank order, the head first
        w = np.array([m["score"] for m in members])
        aux = np.stack([np.concatenate([m["box"], m["full"]]) for m in members])
        c, X, d, av, _, _ = fuse64([fit64(m["verts"]) for m in members], w, aux)
        want.append(dict(cls=obj, size=len(members), score=w.sum() / 3.0, centre=c, pose=X.T, dims=d[[2, 1, 0]], verts=c + (boxgen.UNIT * d) @ X,
                         box=av[:4], full=av[4:], c2d=_project(c, K_IMG)))
    want.sort(key=lambda r: -r["score"])
    return views, raws, want


def _planted_views(dev):
    from omni3d_amd.cubercnn.config import add_tta_config, get_cfg_defaults
    from omni3d_amd.cubercnn.modeling.meta_arch.tta import RCNN3DWithTTA
    from omni3d_amd.d2.config import get_cfg
    views, raws, want = _planted(dev)
    cfg = get_cfg()
    get_cfg_defaults(cfg)
    add_tta_config(cfg)
    cfg.merge_from_list(["TEST.AUG.ENABLED", True, "TEST.AUG.MIN_SIZES", (32, 40), "TEST.AUG.FLIP", True, "TEST.DETECTIONS_PER_IMAGE", 10])
    seen = []

    class Planted(RCNN3DWithTTA):
        def infer_view(self, view_inputs):
            seen.append(view_inputs)
            return raws[len(seen) - 1]

    wrapper = Planted(cfg, _StubModel(dev)).eval()
    assert wrapper.views == [(32, False), (32, True), (40, False), (40, True)]
    wrapper.views = [(32, False), (32, True), (40, False)]           # the three planted views
    image = torch.from_numpy(np.random.default_rng(1).integers(0, 255, size=(3, 32, 48), dtype=np.uint8)).to(dev)
    inputs = [{"image": image, "height": H_IMG, "width": W_IMG, "K": K_IMG}]
    out = wrapper(inputs)
    assert len(out) == 1 and len(seen) == 3
    # what each view was given: the image at the view's size, mirrored on the device for the flipped view, with the mirrored intrinsics
    from omni3d_amd.kernels import resize
    for v, got in zip(views, seen):
        assert tuple(got[0]["image"].shape[-2:]) == v["size"] and got[0]["height"] == H_IMG and got[0]["width"] == W_IMG
        assert np.asarray(got[0]["K"])[0][2] == (W_IMG - K_IMG[0][2] if v["flip"] else K_IMG[0][2])
    assert seen[0][0]["image"] is image
    assert torch.equal(seen[1][0]["image"], torch.flip(image, dims=[2]))
    assert torch.equal(seen[2][0]["image"], resize.resize_bilinear_u8(image, 40, 60))
    inst = out[0]["instances"]
    assert inst.image_size == (H_IMG, W_IMG) and len(inst) == 3
    g = {k: getattr(inst, k).cpu().numpy().astype(np.float64) for k in ("scores", "scores_full", "pred_bbox3D", "pred_center_cam", "pred_center_2D",
                                                                       "pred_dimensions", "pred_pose")}
    g["box"], g["cls"] = inst.pred_boxes.tensor.cpu().numpy().astype(np.float64), inst.pred_classes.cpu().numpy()
    assert [w["size"] for w in want] in ([3, 3, 2], [3, 2, 3], [2, 3, 3]) and g["cls"].tolist() == [w["cls"] for w in want]
    for r, w in enumerate(want):
        assert abs(g["scores"][r] - w["score"]) <= REL_TOL * w["score"]
        assert np.abs(g["pred_bbox3D"][r] - w["verts"]).max() <= POS_TOL and np.abs(g["pred_center_cam"][r] - w["centre"]).max() <= POS_TOL
        assert np.abs(g["pred_dimensions"][r] / w["dims"] - 1.0).max() <= REL_TOL and np.abs(g["pred_pose"][r] - w["pose"]).max() <= REL_TOL
        assert np.abs(g["box"][r] - w["box"]).max() <= PIX_TOL and np.abs(g["pred_center_2D"][r] - w["c2d"]).max() <= PIX_TOL
        assert np.abs(g["scores_full"][r] - w["full"]).max() <= REL_TOL
        assert abs(np.linalg.det(g["pred_pose"][r]) - 1.0) <= 1e-5
    two = [w for w in want if w["size"] == 2][0]
    assert two["cls"] == 2                                            # the object one view missed: (s1 + s2) / 3
    # oracle2D inputs are refused; more slots than the kernel holds are refused when the wrapper is built
    with pytest.raises(ValueError, match="oracle2D"):
        wrapper([dict(inputs[0], oracle2D={})])
    cfg.merge_from_list(["TEST.AUG.MIN_SIZES", tuple(range(100, 100 + 129))])
    with pytest.raises(ValueError, match="1024"):
        Planted(cfg, _StubModel(dev))                                 # 129 sizes x 2 x 4 slots = 1032


def test_planted_views_emulated(emu_lib):
    _planted_views("cpu")


@pytest.mark.gpu
def test_planted_views_gpu(hip_lib):
    _planted_views("cuda")
