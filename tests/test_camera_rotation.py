"""INPUT.CAMERA_ROTATION: the geometry helpers, the config node and the training mapper.  The central check paints marks at the projected
corners of cuboids and finds them again, after the rotation (and a crop, and a flip), at the keypoints the mapper returns: pixels, camera
and 3D targets belong together.  Host path, device path over the emulated library, and GPU."""
import copy

import numpy as np
import pytest
import torch

import ref_augment as ref
from test_mapper_augment import H, K0, W, _anno, _at, _Calls, _cfg, _crop, _generic_record, _mapper, _record, _same_state

ANGLES = (4.0, -2.0, 3.0)                          # roll, pitch, yaw of the fixed-angle checks


def _rcfg(*pairs, rot=None, jitter=None, enabled=True):
    from omni3d_amd.cubercnn.config import add_camera_rotation_config
    cfg = _cfg(*pairs, jitter=jitter)
    add_camera_rotation_config(cfg)
    cfg.merge_from_list(["INPUT.CAMERA_ROTATION.ENABLED", enabled] + [v for kv in (rot or {}).items() for v in ("INPUT.CAMERA_ROTATION." + kv[0], kv[1])])
    return cfg


def _fixed(angles=ANGLES, **more):
    return dict({"ROLL": [angles[0]] * 2, "PITCH": [angles[1]] * 2, "YAW": [angles[2]] * 2, "FILL": [0, 0, 0]}, **more)


def _Q(angles=ANGLES):
    from omni3d_amd.d2.data import camera_rotation
    return camera_rotation(*angles)


# ---- geometry -----------------------------------------------------------------------------------------------------------------------------
def test_camera_rotation_is_a_rotation():
    from omni3d_amd.d2.data import camera_rotation
    for angles in ((0, 0, 0), (5, 0, 0), (0, -3, 0), (0, 0, 4), (5, -3, 4), (-15, 15, -15), (0.3, 14.9, -7.7)):
        Q = camera_rotation(*angles)
        assert Q.dtype == np.float64 and Q.shape == (3, 3)
        assert np.abs(Q @ Q.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(Q) - 1.0) <= 1e-12
    assert np.array_equal(camera_rotation(0, 0, 0), np.eye(3))
    for r in (5.0, -12.0):
        Q = camera_rotation(r, 0, 0)                                 # a roll turns about the optical axis: z stays
        assert np.array_equal(Q[2], [0, 0, 1]) and np.array_equal(Q[:, 2], [0, 0, 1])
        assert np.allclose((Q @ [1.0, 2.0, 7.0])[2], 7.0, rtol=0, atol=1e-15)
    # the composition order: Rz(roll) @ Ry(yaw) @ Rx(pitch)
    Q = camera_rotation(5, -3, 4)
    assert np.abs(Q - camera_rotation(5, 0, 0) @ camera_rotation(0, 0, 4) @ camera_rotation(0, -3, 0)).max() <= 1e-15
    # x right, y down, z forward: a positive yaw moves a point straight ahead to the right (+x), a positive pitch moves it up (-y),
    # a positive roll moves a point on the right (+x) down (+y)
    assert (camera_rotation(0, 0, 4) @ [0, 0, 1.0])[0] > 0 and (camera_rotation(0, 3, 0) @ [0, 0, 1.0])[1] < 0
    assert (camera_rotation(5, 0, 0) @ [1.0, 0, 0])[1] > 0


def test_homography_and_points_agree():
    from omni3d_amd.d2.data import homography_apply, rotation_homography
    rs = np.random.RandomState(0)
    for angles in ((5, -3, 4), (-15, 15, 15), (0, 0, 0)):
        Q = _Q(angles)
        Hm, Hinv = rotation_homography(K0, Q)
        assert Hm.dtype == Hinv.dtype == np.float64
        assert np.abs(Hm @ Hinv - np.eye(3)).max() <= 1e-9
        X = np.stack([rs.uniform(-3, 3, 200), rs.uniform(-2, 2, 200), rs.uniform(4, 30, 200)], 1)       # in front of the camera
        assert ((X @ Q.T)[:, 2] > 0).all()
        moved, den = homography_apply(Hm, ref.project(K0, X))
        assert (den > 0).all() and np.abs(moved - ref.project(K0, X @ Q.T)).max() <= 1e-9


# ---- image against targets ----------------------------------------------------------------------------------------------------------------
# centre, dims, category: two deep cuboids (they intersect, which no check minds) whose sixteen projected corners stand 12 px apart
CUBOIDS = [((0.5, 0.1, 5.2), (1.5, 1.8, 3.3), 2), ((-0.3, 0.1, 5.4), (1.5, 1.7, 3.3), 5)]


def _marked_record():
    """a black image with a white 3 x 3 mark on the pixel that holds each projected cuboid corner"""
    annos = [_anno(c, d, cat) for c, d, cat in CUBOIDS]
    rec = _record(annos)
    img = np.zeros((H, W, 3), np.uint8)
    pts = np.concatenate([ref.project(K0, a["bbox3D_cam"]) for a in annos])
    cells = np.floor(pts).astype(int)                                # pixel (col, row) holding the point; its centre is cell + 0.5
    for cx, cy in cells:
        assert 2 <= cx < W - 2 and 2 <= cy < H - 2
        img[cy - 1:cy + 2, cx - 1:cx + 2] = 255
    d = np.abs(cells[:, None] - cells[None]).max(axis=2) + 100 * np.eye(len(cells), dtype=int)
    assert d.min() >= 12, "the marks stand apart, so that a window around one holds no other"
    rec["image_array"] = img
    return rec, annos


def _centroid(image, x, y, radius=5):
    """intensity centroid (continuous pixel coordinates, pixel centres at +0.5) of the window of `radius` around (x, y), None when the
    window leaves the image or is dark"""
    g = image.astype(np.float64).sum(axis=0)
    cx, cy = int(np.floor(x)), int(np.floor(y))
    if cx - radius < 0 or cy - radius < 0 or cx + radius + 1 > g.shape[1] or cy + radius + 1 > g.shape[0]:
        return None
    win = g[cy - radius:cy + radius + 1, cx - radius:cx + radius + 1]
    if win.sum() < 3 * 255 * 4:                                      # less than four white pixels' worth: cut by the frame or a border
        return None
    ys, xs = np.mgrid[cy - radius:cy + radius + 1, cx - radius:cx + radius + 1]
    return np.array([(win * (xs + 0.5)).sum(), (win * (ys + 0.5)).sum()]) / win.sum()


def _marks_and_targets(device):
    rec, annos = _marked_record()
    Q = _Q()
    moved = [np.asarray(a["bbox3D_cam"]) @ Q.T for a in annos]
    for m in moved:                                                  # the fixture: every rotated corner stays inside the frame
        uv = ref.project(K0, m)
        assert (uv[:, 0] > 6).all() and (uv[:, 0] < W - 6).all() and (uv[:, 1] > 6).all() and (uv[:, 1] < H - 6).all(), uv
    seen = set()
    runs = [((), 0, False)] + [(tuple(_crop("absolute", (90, 120))) + ("INPUT.RANDOM_FLIP", "horizontal"), seed, True) for seed in range(1, 7)]
    for pairs, seed, cropped in runs:
        out = _mapper(_rcfg(*pairs, rot=_fixed()), device, seed)(rec)
        inst, image = out["instances"], out["image"].cpu().numpy()
        assert out["camera_rotation"] == Q.tolist() and len(inst) == 2
        x0, y0, cw, ch = out.get("crop", (0, 0, W, H))
        assert tuple(image.shape) == (3, ch, cw) and (out["height"], out["width"]) == (ch, cw)
        assert out["K"] == [[150.0, 0.0, 83.5 - x0], [0.0, 150.0, 57.25 - y0], [0.0, 0.0, 1.0]], "the rotation leaves K alone"
        flipped = float(inst.gt_poses[0, 0, 0]) < 0
        seen.add((cropped, flipped))
        mirror = (lambda uv: np.stack([cw - uv[:, 0], uv[:, 1]], 1)) if flipped else (lambda uv: uv)
        found = 0
        for row, (a, m) in enumerate(zip(annos, moved)):
            c = Q @ np.asarray(a["center_cam"])
            want_k = mirror(ref.project(out["K"], m))                # through the RETURNED camera
            got_k = inst.gt_keypoints.tensor[row, :, :2].numpy().astype(np.float64)
            assert np.abs(got_k - want_k).max() <= 1e-4, (seed, row)
            assert np.abs(inst.gt_boxes3D[row, :2].numpy() - mirror(ref.project(out["K"], [c]))[0]).max() <= 1e-4
            assert np.abs(inst.gt_boxes3D[row, 6:9].numpy() - c).max() <= 1e-6 and abs(float(inst.gt_boxes3D[row, 2]) - c[2]) <= 1e-6
            assert inst.gt_boxes3D[row, 3:6].tolist() == pytest.approx(a["dimensions"])
            pose = Q @ np.asarray(a["pose"])
            if flipped:
                pose = np.diag([1.0, -1.0, -1.0]) @ pose @ np.diag([-1.0, -1.0, 1.0])        # the mapper's mirror of a pose
            assert np.abs(inst.gt_poses[row].numpy() - pose).max() <= 1e-6
            for k in range(8):
                at = _centroid(image, *got_k[k])
                if at is None:
                    assert cropped, "without a crop every mark is in the frame"
                    continue
                found += 1
                assert np.abs(at - got_k[k]).max() <= 1.0, (seed, row, k, at, got_k[k])
        assert found == 16 if not cropped else found >= 4, (seed, found)
    assert seen >= {(False, False), (True, False), (True, True)}


def _boxes_2d(device):
    """the `_anno` records' box is the hull of the projected corners: the rotated box holds the rotated cuboid's projected hull, and is
    the clipped hull of its own four corners moved by Hm"""
    from omni3d_amd.d2.data import homography_apply, rotation_homography
    rec = _generic_record()
    Q = _Q()
    Hm = rotation_homography(K0, Q)[0]
    out = _mapper(_rcfg(rot=_fixed()), device, 0)(rec)
    inst = out["instances"]
    assert len(inst) == 3
    for row, a in enumerate(rec["annotations"]):
        x0, y0, x1, y1 = a["bbox"]
        uv, den = homography_apply(Hm, [(x0, y0), (x1, y0), (x0, y1), (x1, y1)])
        assert (den > 0).all()
        want = [np.clip(uv[:, 0], 0, W).min(), np.clip(uv[:, 1], 0, H).min(), np.clip(uv[:, 0], 0, W).max(), np.clip(uv[:, 1], 0, H).max()]
        got = inst.gt_boxes.tensor[row].numpy().astype(np.float64)
        assert np.abs(got - want).max() <= 1e-4, (row, got, want)
        hull = ref.project(K0, np.asarray(a["bbox3D_cam"]) @ Q.T)
        hx, hy = np.clip(hull[:, 0], 0, W), np.clip(hull[:, 1], 0, H)
        assert got[0] <= hx.min() + 1e-4 and got[1] <= hy.min() + 1e-4 and got[2] >= hx.max() - 1e-4 and got[3] >= hy.max() - 1e-4, row


def _dropping(device):
    """a 15 degree yaw moves the picture by about 150 * tan(15 deg) = 40 px: a small object at the edge it moves towards leaves the frame
    and is dropped, one that ends across the border is clipped to it, one in the middle is kept whole"""
    from omni3d_amd.d2.data import homography_apply, rotation_homography
    angles = (0.0, 0.0, 15.0)
    Hm = rotation_homography(K0, _Q(angles))[0]
    shift = homography_apply(Hm, [(W / 2, H / 2)])[0][0, 0] - W / 2
    assert 30 < abs(shift) < 50
    edge = W - 12 if shift > 0 else 12                               # the side the picture moves towards
    annos = [_anno(_at(edge, 60, 10.0), (0.4, 0.4, 0.4), 1), _anno(_at(edge - np.sign(shift) * 38, 60, 10.0), (1.2, 0.8, 0.8), 2),
             _anno(_at(80, 60, 10.0), (0.5, 0.5, 0.5), 3)]
    for a, gone, cut in zip(annos, (True, False, False), (False, True, False)):   # the float64 reference decides what the fixture is
        uv = homography_apply(Hm, [(a["bbox"][0], a["bbox"][1]), (a["bbox"][2], a["bbox"][3])])[0]
        lo, hi = uv[:, 0].min(), uv[:, 0].max()
        assert (lo >= W or hi <= 0) == gone and ((lo < W < hi) or (lo < 0 < hi)) == cut, (lo, hi)
    out = _mapper(_rcfg(rot=_fixed(angles)), device, 0)(_record(annos))
    inst = out["instances"]
    assert inst.gt_classes.tolist() == [2, 3]
    box = inst.gt_boxes.tensor[0].tolist()
    assert (box[2] == W and box[0] < W) if shift > 0 else (box[0] == 0 and box[2] > 0)
    assert 0 < inst.gt_boxes.tensor[1, 0] and inst.gt_boxes.tensor[1, 2] < W
    # a centre that goes behind the camera, and a box corner whose denominator is not positive, drop the annotation as well
    from omni3d_amd.cubercnn.data import rotate_instance_annotations
    behind = _anno((9.0, 0.0, 0.5), (0.2, 0.2, 0.2), 1)
    behind["bbox"] = [150.0, 50.0, 158.0, 60.0]
    Q = _Q((0.0, 0.0, 15.0))
    assert (Q @ behind["center_cam"])[2] <= 0 < behind["center_cam"][2]
    done = rotate_instance_annotations(copy.deepcopy(behind), Q, np.array(K0), H, W)
    assert done["bbox"] == [0.0, 0.0, 0.0, 0.0] and done["center_cam"] == behind["center_cam"]
    wide = np.array([[2.0, 0.0, 80.0], [0.0, 2.0, 60.0], [0.0, 0.0, 1.0]])
    far = _anno((0.0, 0.0, 5.0), (0.2, 0.2, 0.2), 1)
    far["bbox"] = [140.0, 50.0, 160.0, 70.0]
    assert (homography_apply(rotation_homography(wide, _Q((0, 0, 15.0)))[0], [(160.0, 50.0)])[1] <= 0).all()
    assert rotate_instance_annotations(far, _Q((0, 0, 15.0)), wide, H, W)["bbox"] == [0.0, 0.0, 0.0, 0.0]


# ---- draws --------------------------------------------------------------------------------------------------------------------------------
def _draws(device):
    rec = _generic_record()
    crop = _crop("relative_range", (0.5, 0.7))
    base = crop + ["INPUT.MIN_SIZE_TRAIN", (48, 90, 131), "INPUT.RANDOM_FLIP", "horizontal"]
    jitter = {"BRIGHTNESS": [0.6, 1.4], "CONTRAST": [1, 1], "SATURATION": [0.5, 2.0]}
    for rot, drawn in (({"ROLL": [-5, 5], "PITCH": [-3, 3], "YAW": [-2, 2]}, (1, 1, 1)), ({}, (1, 1, 0)), ({"PITCH": [1.5, 1.5]}, (1, 0, 0)),
                       ({"ROLL": [2, 2], "PITCH": [0, 0], "YAW": [-1.0, -1.0]}, (0, 0, 0))):
        iv = [rot.get(k, d) for k, d in (("ROLL", [-5, 5]), ("PITCH", [-3, 3]), ("YAW", [0, 0]))]
        for seed in range(3):
            replay = np.random.RandomState(seed)
            angles = [replay.uniform(lo, hi) if d else float(lo) for (lo, hi), d in zip(iv, drawn)]       # roll, pitch, yaw
            box = ref.crop_box(H, W, "relative_range", (0.5, 0.7), replay)                               # then the crop's draws
            replay.choice((48, 90, 131))                                                                 # the size
            replay.uniform()                                                                             # the flip
            replay.uniform(0.6, 1.4), replay.uniform(0.5, 2.0)                                           # the jitter's
            m = _mapper(_rcfg(*base, rot=rot, jitter=jitter), device, seed)
            out = m(rec)
            assert _same_state(m.rng, replay), (rot, seed)
            assert out["camera_rotation"] == _Q(angles).tolist() and out["crop"] == box


def _off_is_the_parent(device):
    """ENABLED False after add_camera_rotation_config: the output, the library calls and the stream of a cfg that never heard of it"""
    rec = _generic_record()
    pairs = _crop("relative_range", (0.5, 0.7)) + ["INPUT.MIN_SIZE_TRAIN", (48, 90, 131), "INPUT.RANDOM_FLIP", "horizontal"]
    for p in ((), pairs):
        for seed in range(3):
            a, b = _mapper(_cfg(*p, jitter={}), device, seed), _mapper(_rcfg(*p, jitter={}, enabled=False, rot={"ROLL": [3, 3]}), device, seed)
            assert b.rotation is None
            with _Calls(device) as calls_a:
                out_a = a(rec)
            with _Calls(device) as calls_b:
                out_b = b(rec)
            assert calls_a == calls_b and _same_state(a.rng, b.rng) and "camera_rotation" not in out_b and b.rotation_skipped == 0
            assert torch.equal(out_a["image"], out_b["image"]) and sorted(out_a) == sorted(out_b)
            assert (out_a["K"], out_a["height"], out_a["width"], out_a.get("crop")) == (out_b["K"], out_b["height"], out_b["width"], out_b.get("crop"))
            ia, ib = out_a["instances"], out_b["instances"]
            for f in ("gt_classes", "gt_boxes3D", "gt_poses"):
                assert torch.equal(getattr(ia, f), getattr(ib, f)), f
            assert torch.equal(ia.gt_boxes.tensor, ib.gt_boxes.tensor) and torch.equal(ia.gt_keypoints.tensor, ib.gt_keypoints.tensor)


# ---- paths --------------------------------------------------------------------------------------------------------------------------------
def _paths(device):
    """host and device mappers give the same bytes; the device path is the warp, then the plain resize -- under a crop too"""
    from omni3d_amd.cubercnn.data.dataset_mapper import warp_homography_u8_host
    from omni3d_amd.d2.data import rotation_homography
    rec = _generic_record()
    crop = _crop("relative_range", (0.5, 0.6))
    for pairs in ([], crop):
        cfg = _rcfg(*pairs, "INPUT.MIN_SIZE_TRAIN", (64, 100, 150), "INPUT.RANDOM_FLIP", "horizontal", rot={"YAW": [-4, 4]}, jitter={"SATURATION": [0.0, 3.0]})
        host, dev = _mapper(cfg, None, 9), _mapper(cfg, device, 9)
        for _ in range(4):
            a = host(rec)
            with _Calls(device) as calls:
                b = dev(rec)
            assert calls == ["omni_warp_homography_u8", "omni_resize_bilinear_u8", "omni_color_jitter_u8"]
            assert b["image"].device.type == device.type and torch.equal(a["image"], b["image"].cpu())
            assert (a["K"], a["height"], a["width"], a.get("crop"), a["camera_rotation"]) == (b["K"], b["height"], b["width"], b.get("crop"), b["camera_rotation"])
            ia, ib = a["instances"], b["instances"]
            assert len(ia) == len(ib) and torch.equal(ia.gt_boxes.tensor, ib.gt_boxes.tensor) and torch.equal(ia.gt_boxes3D, ib.gt_boxes3D)
        assert _same_state(host.rng, dev.rng)
    # the pixels are the definition's: default FILL = the rounded pixel mean, the full frame warped by Hinv, no resize, no flip
    out = _mapper(_rcfg(rot={"ROLL": [4, 4], "PITCH": [-2, -2], "YAW": [3, 3]}), device, 0)(rec)
    want = warp_homography_u8_host(rec["image_array"].transpose(2, 0, 1), rotation_homography(K0, _Q())[1], H, W, (104, 116, 124))
    assert np.array_equal(out["image"].cpu().numpy(), want)
    assert (want == np.array([104, 116, 124], np.uint8)[:, None, None]).all(axis=0).any(), "some border shows"
    # and under a crop the window of that image
    m = _mapper(_rcfg(*_crop("absolute", (70, 90)), rot=_fixed(FILL=[9, 8, 7])), device, 3)
    out = m(rec)
    x0, y0, cw, ch = out["crop"]
    Hinv = rotation_homography(K0, _Q())[1]
    shift = np.array([[1.0, 0.0, x0], [0.0, 1.0, y0], [0.0, 0.0, 1.0]])
    got = out["image"].cpu().numpy()
    assert (ch, cw) == (70, 90) and np.array_equal(got, warp_homography_u8_host(rec["image_array"].transpose(2, 0, 1), Hinv @ shift, ch, cw, (9, 8, 7)))
    # which is the window of the rotated full frame, up to the few pixels where the two matrices' roundings part a weight or the border
    full = warp_homography_u8_host(rec["image_array"].transpose(2, 0, 1), Hinv, H, W, (9, 8, 7))
    assert (got != full[:, y0:y0 + ch, x0:x0 + cw]).mean() < 0.01


def _test_mapper_ignores(device):
    rec = _generic_record()
    a, b = _mapper(_rcfg("INPUT.MIN_SIZE_TEST", 96, rot=_fixed()), device, 0, is_train=False), _mapper(_cfg("INPUT.MIN_SIZE_TEST", 96), device, 0, is_train=False)
    with _Calls(device) as calls:
        out_a = a(rec)
    out_b = b(rec)
    assert calls == ([] if device is None else ["omni_resize_bilinear_u8"]) and a.rotation is None
    assert torch.equal(out_a["image"], out_b["image"]) and "camera_rotation" not in out_a and _same_state(a.rng, b.rng)


def _guard(device):
    """fx = 2 on a 160-wide image: a 15 degree yaw puts the warp's denominator below zero at one side -- the image is left as it is"""
    from omni3d_amd.d2.data import rotation_homography
    from omni3d_amd.kernels.augment import warp_denominator_positive
    wide = [[2.0, 0.0, 80.0], [0.0, 2.0, 60.0], [0.0, 0.0, 1.0]]
    assert not warp_denominator_positive(rotation_homography(wide, _Q((0, 0, 15.0)))[1], H, W)
    rec = _record([_anno(_at(80, 60, 10.0), (0.5, 0.5, 0.5), 3)])
    rec["K"] = wide
    m = _mapper(_rcfg(rot=_fixed((0.0, 0.0, 15.0))), device, 0)
    with _Calls(device) as calls:
        out = m(rec)
    assert m.rotation_skipped == 1 and out["camera_rotation"] == np.eye(3).tolist()
    assert calls == ([] if device is None else ["omni_resize_bilinear_u8"])
    assert np.array_equal(out["image"].cpu().numpy(), rec["image_array"].transpose(2, 0, 1)) and len(out["instances"]) == 1
    assert out["instances"].gt_boxes3D[0, 6:9].tolist() == pytest.approx(rec["annotations"][0]["center_cam"])
    m(_generic_record())                                             # a sane camera next: rotated, not counted
    assert m.rotation_skipped == 1


CHECKS = [_marks_and_targets, _boxes_2d, _dropping, _draws, _off_is_the_parent, _test_mapper_ignores, _guard]
_ids = [f.__name__.strip("_") for f in CHECKS]


@pytest.mark.parametrize("check", CHECKS, ids=_ids)
def test_rotation_host(check):
    check(None)


@pytest.mark.parametrize("check", CHECKS + [_paths], ids=_ids + ["paths"])
def test_rotation_emulated(emu_lib, check):
    check(torch.device("cpu"))


@pytest.mark.gpu
@pytest.mark.parametrize("check", CHECKS + [_paths], ids=_ids + ["paths"])
def test_rotation_gpu(hip_lib, check):
    check(torch.device("cuda"))


# ---- config -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", [{"ROLL": [3, -3]}, {"PITCH": [-16, 0]}, {"YAW": [0, 16]}, {"ROLL": [1.0]}, {"PITCH": [-1, 0, 1]}, {"YAW": []},
                                 {"ROLL": [0, float("nan")]}, {"FILL": [1, 2]}, {"FILL": [0, 0, 256]}, {"FILL": [0.5, 0, 0]}], ids=str)
def test_bad_rotation_config_is_refused_at_construction(rot):
    from omni3d_amd.cubercnn.config import camera_rotation_args
    with pytest.raises(ValueError):
        _mapper(_rcfg(rot=rot), None, 0)
    with pytest.raises(ValueError):
        camera_rotation_args(_rcfg(rot=rot))


def test_camera_rotation_config_is_off_by_default_and_idempotent():
    from omni3d_amd.cubercnn.config import add_camera_rotation_config, camera_rotation_args
    cfg = _cfg()
    assert "CAMERA_ROTATION" not in cfg.INPUT and camera_rotation_args(cfg)["enabled"] is False
    assert _mapper(cfg, None, 0).rotation is None
    add_camera_rotation_config(cfg)
    assert dict(cfg.INPUT.CAMERA_ROTATION) == {"ENABLED": False, "ROLL": [-5.0, 5.0], "PITCH": [-3.0, 3.0], "YAW": [0.0, 0.0], "FILL": []}
    assert _mapper(cfg, None, 0).rotation is None
    cfg.merge_from_list(["INPUT.CAMERA_ROTATION.ENABLED", True, "INPUT.CAMERA_ROTATION.PITCH", [-1.0, 2.0]])
    add_camera_rotation_config(cfg)
    # FILL []: MODEL.PIXEL_MEAN (103.53, 116.28, 123.675, in INPUT.FORMAT order) rounded to the nearest byte
    assert camera_rotation_args(cfg) == {"enabled": True, "roll": (-5.0, 5.0), "pitch": (-1.0, 2.0), "yaw": (0.0, 0.0), "fill": (104, 116, 124)}
    m = _mapper(cfg, None, 0)
    assert m.rotation == ((-5.0, 5.0), (-1.0, 2.0), (0.0, 0.0)) and m.rotation_fill == (104, 116, 124) and m.rotation_skipped == 0
    cfg.merge_from_list(["INPUT.CAMERA_ROTATION.FILL", [1, 2, 3], "MODEL.PIXEL_MEAN", [0.4, 254.5, 300.0]])
    assert camera_rotation_args(cfg)["fill"] == (1, 2, 3)
    cfg.merge_from_list(["INPUT.CAMERA_ROTATION.FILL", []])
    assert camera_rotation_args(cfg)["fill"] == (0, 255, 255)
    assert _mapper(_rcfg(enabled=False), None, 0, is_train=False).rotation is None


def test_a_record_without_a_camera_is_refused():
    rec = _generic_record()
    del rec["K"]
    with pytest.raises(ValueError, match="K"):
        _mapper(_rcfg(rot=_fixed()), None, 0)(rec)


# ---- tools/show_augment.py ----------------------------------------------------------------------------------------------------------------
def test_show_augment_draws_rotated_cuboids_on_their_objects(emu_lib):
    """one off-centre cuboid on a black image under a drawn rotation: what tools/show_augment.py paints through the returned camera lies
    inside the instance's rotated 2D box and around its projected centre"""
    from test_show_augment import _tool
    tool = _tool()
    rec = {"image_array": np.zeros((H, W, 3), np.uint8), "height": H, "width": W, "K": copy.deepcopy(K0), "image_id": 1, "dataset_id": 0,
           "file_name": "memory://1", "annotations": [_anno(_at(45, 55, 8.0), (1.0, 1.2, 0.8), 1)]}
    mapper = _mapper(_rcfg(rot={"ROLL": [-5, 5], "PITCH": [-3, 3], "YAW": [-4, 4], "FILL": [0, 0, 0]}), torch.device("cpu"), 0)
    moved = set()
    for _ in range(4):
        out = mapper(rec)
        inst = out["instances"]
        assert len(inst) == 1
        K, boxes = tool.camera_and_cuboids(out)
        u, v = inst.gt_boxes3D[0, :2].tolist()
        moved.add((round(u), round(v)))
        assert np.allclose(boxes[0][:3], inst.gt_boxes3D[0, 6:9].tolist(), atol=1e-4), "the back-projected centre is the rotated centre"
        im, n = tool.draw_record(out, "BGR")
        ys, xs = np.nonzero(im.any(axis=2))
        x1, y1, x2, y2 = inst.gt_boxes.tensor[0].tolist()
        assert n == 1 and len(xs) > 20
        assert x1 - 3 <= xs.min() and xs.max() <= x2 + 3 and y1 - 3 <= ys.min() and ys.max() <= y2 + 3
        assert xs.min() < u < xs.max() and ys.min() < v < ys.max()
    assert len(moved) == 4


def test_show_augment_takes_camera_rotation_pairs(emu_lib, tmp_path, capsys):
    """`tools/show_augment.py DATASET.json OUT INPUT.CAMERA_ROTATION.ENABLED True` over a synthetic on-disk dataset: the images are
    written at their size, and they differ from the unrotated ones"""
    from PIL import Image
    from omni3d_amd import synthetic
    from omni3d_amd.d2.data import MetadataCatalog
    from test_show_augment import NAMES, _tool
    path = synthetic.write_omni3d_dataset(str(tmp_path), "Synth_train", NAMES, [5, 2, 9], num_images=2, height=96, width=128, num_gt=3, seed=6)
    saved = {k: MetadataCatalog.get(k) for k in ("omni3d_model", "Synth_train") if k in MetadataCatalog}
    still = ["INPUT.MIN_SIZE_TRAIN", "(0,)", "INPUT.RANDOM_FLIP", "none"]
    try:
        tool = _tool()
        turned = tool.main([path, str(tmp_path / "turned"), "--n", "2", "INPUT.CAMERA_ROTATION.ENABLED", "True", "INPUT.CAMERA_ROTATION.ROLL", "[5,5]"] + still)
        plain = tool.main([path, str(tmp_path / "plain"), "--n", "2"] + still)
    finally:
        for k in ("omni3d_model", "Synth_train"):
            MetadataCatalog.pop(k, None)
        MetadataCatalog.update(saved)
    assert len(turned) == len(plain) == 2
    for p, q in zip(turned, plain):
        with Image.open(p) as a, Image.open(q) as b:
            a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape == (96, 128, 3) and (a != b).any(axis=2).mean() > 0.2
    assert sum("cuboids kept" in ln for ln in capsys.readouterr().out.splitlines()) == 4
