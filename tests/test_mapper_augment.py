"""The training `DatasetMapper3D`: its output with the augmentations off (the parent's), and INPUT.CROP / INPUT.COLOR_JITTER -- the draws
against the seeded stream, the pixels against PIL on the slice, and the camera the cropped dict carries against the pinhole
projection in float64.  Every check runs on the host path (PIL + numpy), on the device path over the emulated library, and on the GPU."""
import copy

import numpy as np
import pytest
import torch

H, W = 120, 160
K0 = [[150.0, 0.0, 83.5], [0.0, 150.0, 57.25], [0.0, 0.0, 1.0]]


def _cfg(*pairs, jitter=None):
    from omni3d_amd.cubercnn.config import get_cfg_defaults
    from omni3d_amd.d2.config import get_cfg
    cfg = get_cfg()
    get_cfg_defaults(cfg)
    cfg.merge_from_list(["INPUT.MIN_SIZE_TRAIN", (0,), "INPUT.MIN_SIZE_TRAIN_SAMPLING", "choice", "INPUT.MAX_SIZE_TRAIN", 4000,
                         "INPUT.RANDOM_FLIP", "none"] + list(pairs))
    if jitter is not None:
        from omni3d_amd.cubercnn.config import add_color_jitter_config
        add_color_jitter_config(cfg)
        cfg.merge_from_list(["INPUT.COLOR_JITTER.ENABLED", True] + [v for kv in jitter.items() for v in ("INPUT.COLOR_JITTER." + kv[0], kv[1])])
    return cfg


def _crop(kind, size):
    return ["INPUT.CROP.ENABLED", True, "INPUT.CROP.TYPE", kind, "INPUT.CROP.SIZE", list(size)]


def _mapper(cfg, device, seed, is_train=True):
    from omni3d_amd.cubercnn.data import DatasetMapper3D
    m = DatasetMapper3D(cfg, is_train, device=device, rng=np.random.RandomState(seed))
    m.dataset_id_to_unknown_cats = {0: set()}
    return m


def _cuboid(center, dims):
    c, d = np.asarray(center, np.float64), np.asarray(dims, np.float64) / 2
    return [[c[0] + sx * d[0], c[1] + sy * d[1], c[2] + sz * d[2]] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]


def _anno(center, dims, cat):
    """a cuboid with its 2D box the hull of its projected corners (float64)"""
    from omni3d_amd.d2.structures import BoxMode
    corners = _cuboid(center, dims)
    uv = (np.asarray(corners) @ np.asarray(K0).T)
    uv = uv[:, :2] / uv[:, 2:3]
    eye = np.eye(3).tolist()
    return {"bbox": [uv[:, 0].min(), uv[:, 1].min(), uv[:, 0].max(), uv[:, 1].max()], "bbox_mode": BoxMode.XYXY_ABS, "category_id": cat,
            "center_cam": list(center), "dimensions": list(dims), "pose": eye, "R_cam": copy.deepcopy(eye), "bbox3D_cam": corners,
            "ignore": False, "iscrowd": 0}


def _at(u, v, z):
    """the camera point that K0 projects to pixel (u, v) at depth z"""
    return [(u - K0[0][2]) * z / K0[0][0], (v - K0[1][2]) * z / K0[1][1], z]


def _record(annos=()):
    rs = np.random.RandomState(11)
    img = rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    img[: H // 4] = 255
    img[:, : W // 5] = 0
    return {"image_array": img, "height": H, "width": W, "K": copy.deepcopy(K0), "image_id": 7, "dataset_id": 0, "file_name": "memory://7",
            "annotations": list(annos)}


def _generic_record():
    return _record([_anno(_at(40, 50, 8.0), (1.0, 1.2, 0.8), 1), _anno(_at(100, 70, 12.0), (2.0, 1.5, 1.0), 0), _anno(_at(130, 30, 9.0), (0.7, 0.7, 0.7), 3)])


class _Calls:
    """records the names the mapper passes to the library's `call` on the device path"""

    def __init__(self, device):
        from omni3d_amd import lib
        self.names, self.lib = [], (lib.get() if device is not None else None)

    def __enter__(self):
        if self.lib is not None:
            real = self.lib.call
            self.lib.call = lambda name, *a: (self.names.append(name), real(name, *a))[1]
        return self.names

    def __exit__(self, *exc):
        if self.lib is not None:
            del self.lib.call


def _pil(hwc, nh, nw, flip):
    from PIL import Image
    out = np.asarray(Image.fromarray(np.ascontiguousarray(hwc)).resize((nw, nh), Image.BILINEAR))
    return np.ascontiguousarray((np.flip(out, axis=1) if flip else out).transpose(2, 0, 1))


def _same_state(a, b):
    sa, sb = a.get_state(), b.get_state()
    return sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


# ---- features off: the parent's output, calls and draws (this check passes on the parent as well) -----------------------------------------
def _features_off(device):
    from omni3d_amd.cubercnn.data import transform_instance_annotations
    from omni3d_amd.d2.data import HFlipTransform, NoOpTransform, ResizeTransform, TransformList, resize_shortest_edge_size
    cfg = _cfg("INPUT.MIN_SIZE_TRAIN", (96, 144, 200), "INPUT.RANDOM_FLIP", "horizontal")
    rec = _generic_record()
    seen_flip = set()
    for seed in range(4):
        replay = np.random.RandomState(seed)
        nh, nw = resize_shortest_edge_size(H, W, (96, 144, 200), 4000, "choice", replay)           # draw 1: the size
        flip = replay.uniform() < 0.5                                                              # draw 2: the flip
        seen_flip.add(bool(flip))
        m = _mapper(cfg, device, seed)
        with _Calls(device) as calls:
            out = m(rec)
        assert calls == ([] if device is None else ["omni_resize_bilinear_u8"])
        assert _same_state(m.rng, replay), "the mapper drew more or less than (size, flip)"
        assert out["image"].dtype == torch.uint8 and np.array_equal(out["image"].cpu().numpy(), _pil(rec["image_array"], nh, nw, flip))
        assert out["K"] == K0 and (out["height"], out["width"]) == (H, W) and "crop" not in out and "image_array" not in out
        tfm = TransformList([ResizeTransform(H, W, nh, nw), HFlipTransform(nw) if flip else NoOpTransform()])
        annos = [transform_instance_annotations(a, tfm, K=np.array(K0)) for a in copy.deepcopy(rec["annotations"])]
        inst = out["instances"]
        assert inst.image_size == (nh, nw) and len(inst) == 3
        assert inst.gt_classes.tolist() == [1, 0, 3]
        assert torch.equal(inst.gt_boxes.tensor, torch.tensor(np.asarray([a["bbox"] for a in annos], dtype=np.float32)))
        assert torch.equal(inst.gt_boxes3D, torch.FloatTensor([a["center_cam_proj"] + a["dimensions"] + a["center_cam"] for a in annos]))
        assert torch.equal(inst.gt_poses, torch.FloatTensor([a["pose"] for a in annos]))
        assert torch.equal(inst.gt_keypoints.tensor, torch.FloatTensor([a["keypoints"] for a in annos]))
        assert inst.gt_unknown_category_mask.shape == (3, 1) and not bool(inst.gt_unknown_category_mask.any())
    assert seen_flip == {True, False}


# ---- crop sampling ------------------------------------------------------------------------------------------------------------------------
CROPS = [("relative", (0.6, 0.75)), ("relative_range", (0.5, 0.7)), ("absolute", (50, 90)), ("absolute_range", (40, 100)),
         ("absolute", (500, 90)), ("absolute", (500, 700))]        # the last two: larger than the image in one / both directions


def _crop_sampling(device):
    import ref_augment as ref
    rec = _record()
    for kind, size in CROPS:
        m, replay = _mapper(_cfg(*_crop(kind, size)), device, 3), np.random.RandomState(3)
        for _ in range(50):
            want = ref.crop_box(H, W, kind, size, replay)
            replay.choice((0,))                                   # the resize's draw comes after the crop's
            out = m(rec)
            assert out["crop"] == want and (out["height"], out["width"]) == (want[3], want[2]), (kind, size)
            assert tuple(out["image"].shape) == (3, want[3], want[2])
        assert _same_state(m.rng, replay)
    out = _mapper(_cfg(*_crop("absolute", (500, 700))), device, 0)(rec)
    assert out["crop"] == (0, 0, W, H) and out["K"] == K0, "a crop larger than the image is the whole image"


# ---- pixels -------------------------------------------------------------------------------------------------------------------------------
def _pixels(device):
    import ref_augment as ref
    rec = _record()
    img = rec["image_array"]
    crop = _crop("relative_range", (0.4, 0.5))
    for seed in range(3):                                          # no resize: the slice itself
        with _Calls(device) as calls:
            out = _mapper(_cfg(*crop), device, seed)(rec)
        x0, y0, cw, ch = out["crop"]
        assert np.array_equal(out["image"].cpu().numpy(), img[y0:y0 + ch, x0:x0 + cw].transpose(2, 0, 1))
        assert calls == ([] if device is None else ["omni_pil_bilinear_coeffs", "omni_pil_bilinear_coeffs", "omni_crop_resize_u8"])
    cfg = _cfg(*crop, "INPUT.MIN_SIZE_TRAIN", (48, 90, 131), "INPUT.RANDOM_FLIP", "horizontal")
    seen_flip = set()
    for seed in range(6):                                          # crop, resize of the crop's size, flip
        from omni3d_amd.d2.data import resize_shortest_edge_size
        replay = np.random.RandomState(seed)
        x0, y0, cw, ch = ref.crop_box(H, W, "relative_range", (0.4, 0.5), replay)
        nh, nw = resize_shortest_edge_size(ch, cw, (48, 90, 131), 4000, "choice", replay)
        flip = replay.uniform() < 0.5
        seen_flip.add(bool(flip))
        m = _mapper(cfg, device, seed)
        out = m(rec)
        assert out["crop"] == (x0, y0, cw, ch) and _same_state(m.rng, replay)
        assert np.array_equal(out["image"].cpu().numpy(), _pil(img[y0:y0 + ch, x0:x0 + cw], nh, nw, flip)), seed
    assert seen_flip == {True, False}


# ---- geometry -----------------------------------------------------------------------------------------------------------------------------
def _geometry(device):
    """absolute 80 x 100 crop, short edge 80 -> 160: both resize factors are exactly 2, so K scaled by image height / height is the
    camera of the output image to the last bit and the 1e-9 bound is about the arithmetic, not about rounded sizes"""
    import ref_augment as ref
    from omni3d_amd.cubercnn.data import transform_instance_annotations
    from omni3d_amd.d2.data import CropTransform, HFlipTransform, NoOpTransform, ResizeTransform, TransformList
    for flip_mode, seeds in (("none", (0, 1)), ("horizontal", range(2, 10))):
        flipped = set()
        for seed in seeds:
            cfg = _cfg(*_crop("absolute", (80, 100)), "INPUT.MIN_SIZE_TRAIN", (160,), "INPUT.RANDOM_FLIP", flip_mode)
            replay = np.random.RandomState(seed)
            x0, y0, cw, ch = ref.crop_box(H, W, "absolute", (80, 100), replay)
            replay.choice((160,))
            flip = flip_mode == "horizontal" and replay.uniform() < 0.5
            flipped.add(bool(flip))
            # one cuboid inside the crop, one cut by its right edge, one outside it (on the wider of the two side margins)
            u_out = (x0 + cw + W) / 2 if W - (x0 + cw) >= x0 else x0 / 2
            annos = [_anno(_at(x0 + cw / 2, y0 + ch / 2, 10.0), (0.6, 0.6, 0.6), 2), _anno(_at(x0 + cw - 1.5, y0 + ch / 2 + 5, 8.0), (1.2, 0.8, 0.9), 5),
                     _anno(_at(u_out, y0 + ch / 2, 10.0), (0.3, 0.3, 0.3), 4)]
            assert max(W - (x0 + cw), x0) >= 30 and annos[1]["bbox"][0] < x0 + cw < annos[1]["bbox"][2]
            rec = _record(annos)
            m = _mapper(cfg, device, seed)
            out = m(rec)
            assert _same_state(m.rng, replay)
            assert out["crop"] == (x0, y0, cw, ch) and (out["height"], out["width"]) == (ch, cw) == (80, 100)
            assert tuple(out["image"].shape) == (3, 160, 200)
            assert isinstance(out["K"], list) and all(isinstance(r, list) for r in out["K"])
            assert out["K"] == [[150.0, 0.0, 83.5 - x0], [0.0, 150.0, 57.25 - y0], [0.0, 0.0, 1.0]]
            s = out["image"].shape[1] / out["height"]
            Ks = np.diag([s, s, 1.0]) @ np.asarray(out["K"], np.float64)
            mirror = (lambda uv: np.stack([200 - uv[:, 0], uv[:, 1]], 1)) if flip else (lambda uv: uv)
            # the transformed annotations in float64, by the mapper's own list of transforms and the ORIGINAL camera
            tfm = TransformList([CropTransform(x0, y0, cw, ch), ResizeTransform(ch, cw, 160, 200), HFlipTransform(200) if flip else NoOpTransform()])
            done = [transform_instance_annotations(a, tfm, K=np.array(K0)) for a in copy.deepcopy(annos)]
            inst = out["instances"]
            assert inst.gt_classes.tolist() == [2, 5], "the cuboid outside the crop is dropped, the other two are kept"
            for row, a in enumerate(done[:2]):
                want_c = mirror(ref.project(Ks, [a["center_cam"]]))[0]
                want_k = mirror(ref.project(Ks, a["bbox3D_cam"]))
                got_c, got_k = np.asarray(a["center_cam_proj"][:2]), np.asarray(a["keypoints"])[:, :2]
                assert np.all(np.abs(got_c - want_c) <= 1e-9 * (1 + np.abs(want_c))), (seed, row, got_c, want_c)
                assert np.all(np.abs(got_k - want_k) <= 1e-9 * (1 + np.abs(want_k))), (seed, row)
                got32 = inst.gt_boxes3D[row, :2].numpy().astype(np.float64)
                assert np.all(np.abs(got32 - want_c) <= np.spacing(np.abs(want_c).astype(np.float32)).astype(np.float64)), (seed, row, got32, want_c)
                # the full 3D target is the annotation's
                assert torch.equal(inst.gt_boxes3D[row, 2:], torch.FloatTensor([a["center_cam_proj"][2]] + a["dimensions"] + a["center_cam"]))
                assert torch.equal(inst.gt_keypoints.tensor[row], torch.FloatTensor(a["keypoints"]))
                assert torch.equal(inst.gt_poses[row], torch.FloatTensor(a["pose"]))
            # the inside cuboid keeps its box; the cut one is clipped to the image rectangle
            box32 = lambda a: torch.tensor(np.asarray(a["bbox"], dtype=np.float32))      # noqa: E731
            assert torch.equal(inst.gt_boxes.tensor[0], box32(done[0]))
            cut, raw = inst.gt_boxes.tensor[1], box32(done[1])
            assert (raw[2] > 200 or raw[0] < 0) and torch.equal(cut, torch.stack([raw[0].clamp(0, 200), raw[1].clamp(0, 160), raw[2].clamp(0, 200),
                                                                                 raw[3].clamp(0, 160)]))
            assert float(cut[0]) == 0.0 if flip else float(cut[2]) == 200.0
            b = box32(done[2])
            assert b[2] <= 0 or b[0] >= 200, "the third cuboid's box lies outside the output image"
        assert flipped == ({False} if flip_mode == "none" else {True, False})


# ---- jitter -------------------------------------------------------------------------------------------------------------------------------
def _jitter(device):
    import ref_augment as ref
    rec = _record()
    crop = _crop("relative", (0.7, 0.8))
    base = ["INPUT.MIN_SIZE_TRAIN", (100,), "INPUT.RANDOM_FLIP", "horizontal"]
    for fmt, c_red in (("BGR", 2), ("RGB", 0)):
        for jitter, drawn in (({"BRIGHTNESS": [0.6, 1.4], "CONTRAST": [0.5, 1.5], "SATURATION": [0.0, 2.0]}, (1, 1, 1)),
                              ({"BRIGHTNESS": [1, 1], "CONTRAST": [0.5, 1.5], "SATURATION": [1.0, 1.0]}, (0, 1, 0)),
                              ({"BRIGHTNESS": [1.0, 1.0], "CONTRAST": [1, 1], "SATURATION": [1, 1]}, (0, 0, 0)),
                              ({"BRIGHTNESS": [0.5, 0.5], "CONTRAST": [1, 1], "SATURATION": [4, 4]}, (1, 0, 1))):
            for seed in range(3):
                plain = _mapper(_cfg(*crop, *base, "INPUT.FORMAT", fmt), device, seed)(rec)["image"].cpu().numpy()
                replay = np.random.RandomState(seed)
                ref.crop_box(H, W, "relative", (0.7, 0.8), replay)
                replay.choice((100,))
                replay.uniform()
                iv = [jitter[k] for k in ("BRIGHTNESS", "CONTRAST", "SATURATION")]
                w = [ref.weight(replay.uniform(lo, hi)) if d else 4096 for (lo, hi), d in zip(iv, drawn)]    # after the flip, in this order
                m = _mapper(_cfg(*crop, *base, "INPUT.FORMAT", fmt, jitter=jitter), device, seed)
                with _Calls(device) as calls:
                    out = m(rec)
                assert _same_state(m.rng, replay), (jitter, "draws")
                assert np.array_equal(out["image"].cpu().numpy(), ref.color_jitter(plain, *w, c_red)), (fmt, jitter, seed, w)
                if device is not None:
                    assert calls == ["omni_pil_bilinear_coeffs", "omni_pil_bilinear_coeffs", "omni_crop_resize_u8"] + (
                        ["omni_color_jitter_u8"] if w != [4096, 4096, 4096] else [])
    # the jitter alone, on the resized image, with the crop off
    cfg = _cfg("INPUT.MIN_SIZE_TRAIN", (90,), jitter={"CONTRAST": [0.3, 0.3]})
    plain = _mapper(_cfg("INPUT.MIN_SIZE_TRAIN", (90,)), device, 5)(rec)["image"].cpu().numpy()
    replay = np.random.RandomState(5)
    replay.choice((90,))
    w = [ref.weight(replay.uniform(lo, hi)) for lo, hi in ([0.8, 1.2], [0.3, 0.3], [0.8, 1.2])]
    out = _mapper(cfg, device, 5)(rec)
    assert "crop" not in out and np.array_equal(out["image"].cpu().numpy(), ref.color_jitter(plain, *w, 2))


# ---- test mode ----------------------------------------------------------------------------------------------------------------------------
def _test_mode(device):
    rec = _generic_record()
    on = _cfg(*_crop("relative", (0.5, 0.5)), "INPUT.MIN_SIZE_TEST", 96, jitter={"BRIGHTNESS": [0.2, 0.3]})
    off = _cfg("INPUT.MIN_SIZE_TEST", 96)
    a, b = _mapper(on, device, 0, is_train=False), _mapper(off, device, 0, is_train=False)
    with _Calls(device) as calls:
        out_a = a(rec)
    out_b = b(rec)
    assert calls == ([] if device is None else ["omni_resize_bilinear_u8"])
    assert torch.equal(out_a["image"], out_b["image"]) and tuple(out_a["image"].shape) == (3, 96, 128)
    assert "crop" not in out_a and out_a["K"] == K0 and (out_a["height"], out_a["width"]) == (H, W)
    assert _same_state(a.rng, b.rng)


# ---- build_detection_train_loader ---------------------------------------------------------------------------------------------------------
def _loader(device):
    import itertools
    from omni3d_amd import synthetic
    from omni3d_amd.cubercnn.data import build_detection_train_loader
    dicts = synthetic.make_dataset_dicts(num_images=4, height=96, width=128, num_gt=4, seed=2)
    by_id = {d["image_id"]: d for d in dicts}
    cfg = _cfg(*_crop("relative_range", (0.5, 0.6)), "INPUT.MIN_SIZE_TRAIN", (64, 80), "INPUT.RANDOM_FLIP", "horizontal", "SEED", 1,
               jitter={})
    loader = build_detection_train_loader(cfg, mapper=_mapper(cfg, device, 0), dataset=dicts, total_batch_size=2)
    n = 0
    for batch in itertools.islice(iter(loader), 4):
        assert len(batch) == 2
        for d in batch:
            n += 1
            x0, y0, cw, ch = d["crop"]
            src = by_id[d["image_id"]]
            assert 0 <= x0 and 0 <= y0 and x0 + cw <= 128 and y0 + ch <= 96 and (d["height"], d["width"]) == (ch, cw)
            Ksrc, Kd = np.asarray(src["K"], np.float64), np.asarray(d["K"], np.float64)
            assert np.array_equal(Kd - Ksrc, [[0, 0, -x0], [0, 0, -y0], [0, 0, 0]])
            _, nh, nw = d["image"].shape
            assert d["image"].dtype == torch.uint8 and min(nh, nw) in (64, 80) and d["instances"].image_size == (nh, nw)
            assert abs(nh / ch - nw / cw) <= 1.0 / min(ch, cw), "one resize factor up to the rounding of the longer side"
            inst = d["instances"]
            box = inst.gt_boxes.tensor
            assert bool((box[:, 0] >= 0).all() and (box[:, 1] >= 0).all() and (box[:, 2] <= nw).all() and (box[:, 3] <= nh).all())
            assert bool(inst.gt_boxes.nonempty().all()) and inst.gt_boxes3D.shape == (len(inst), 9)
    assert n == 8


CHECKS = [_features_off, _crop_sampling, _pixels, _geometry, _jitter, _test_mode, _loader]
_ids = [f.__name__.strip("_") for f in CHECKS]


@pytest.mark.parametrize("check", CHECKS, ids=_ids)
def test_mapper_host(check):
    check(None)


@pytest.mark.parametrize("check", CHECKS, ids=_ids)
def test_mapper_emulated(emu_lib, check):
    check(torch.device("cpu"))


@pytest.mark.gpu
@pytest.mark.parametrize("check", CHECKS, ids=_ids)
def test_mapper_gpu(hip_lib, check):
    check(torch.device("cuda"))


# ---- host and device mappers agree ----------------------------------------------------------------------------------------------------------
def _host_and_device_agree(device):
    cfg = _cfg(*_crop("relative_range", (0.5, 0.6)), "INPUT.MIN_SIZE_TRAIN", (64, 100, 150), "INPUT.RANDOM_FLIP", "horizontal",
               jitter={"SATURATION": [0.0, 3.0]})
    rec = _generic_record()
    host, dev = _mapper(cfg, None, 9), _mapper(cfg, device, 9)
    for _ in range(6):
        a, b = host(rec), dev(rec)
        assert b["image"].device.type == device.type and torch.equal(a["image"], b["image"].cpu())
        assert (a["K"], a["height"], a["width"], a["crop"]) == (b["K"], b["height"], b["width"], b["crop"])
        ia, ib = a["instances"], b["instances"]
        assert ia.image_size == ib.image_size and len(ia) == len(ib)
        for f in ("gt_classes", "gt_boxes3D", "gt_poses", "gt_unknown_category_mask"):
            assert torch.equal(getattr(ia, f), getattr(ib, f)), f
        assert torch.equal(ia.gt_boxes.tensor, ib.gt_boxes.tensor) and torch.equal(ia.gt_keypoints.tensor, ib.gt_keypoints.tensor)
    assert _same_state(host.rng, dev.rng)


def test_host_and_device_mappers_agree_emulated(emu_lib):
    _host_and_device_agree(torch.device("cpu"))


@pytest.mark.gpu
def test_host_and_device_mappers_agree_gpu(hip_lib):
    _host_and_device_agree(torch.device("cuda"))


# ---- validation at construction -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pairs", [
    _crop("centre", (0.5, 0.5)),                                   # unknown TYPE
    _crop("relative", (0.0, 0.5)), _crop("relative", (0.5, 1.01)), _crop("relative_range", (-0.1, 0.5)), _crop("relative_range", (1.5, 0.5)),
    _crop("relative", (0.5,)), _crop("absolute", (50, 60, 70)), _crop("relative_range", ()),      # wrong length
    _crop("absolute_range", (100, 40)),                            # s0 > s1
], ids=lambda p: "{}-{}".format(p[3], p[5]))
def test_bad_crop_is_refused_at_construction(pairs):
    with pytest.raises(ValueError):
        _mapper(_cfg(*pairs), None, 0)


@pytest.mark.parametrize("jitter", [{"BRIGHTNESS": [-0.1, 1.0]}, {"CONTRAST": [1.2, 0.8]}, {"SATURATION": [0.5, 4.5]}, {"BRIGHTNESS": [1.0]},
                                    {"CONTRAST": [0.5, 1.0, 1.5]}, {"SATURATION": [0.5, float("nan")]}], ids=str)
def test_bad_jitter_interval_is_refused_at_construction(jitter):
    from omni3d_amd.cubercnn.config import color_jitter_args
    with pytest.raises(ValueError):
        _mapper(_cfg(jitter=jitter), None, 0)
    with pytest.raises(ValueError):
        color_jitter_args(_cfg(jitter=jitter))


def test_jitter_needs_a_known_channel_order():
    with pytest.raises(ValueError):
        _mapper(_cfg("INPUT.FORMAT", "YUV-BT.601", jitter={}), None, 0)
    assert _mapper(_cfg("INPUT.FORMAT", "YUV-BT.601"), None, 0).jitter is None


def test_color_jitter_config_is_off_by_default_and_idempotent():
    from omni3d_amd.cubercnn.config import add_color_jitter_config, color_jitter_args
    cfg = _cfg()
    assert "COLOR_JITTER" not in cfg.INPUT and color_jitter_args(cfg)["enabled"] is False
    assert _mapper(cfg, None, 0).jitter is None and _mapper(cfg, None, 0).crop is None
    add_color_jitter_config(cfg)
    assert dict(cfg.INPUT.COLOR_JITTER) == {"ENABLED": False, "BRIGHTNESS": [0.8, 1.2], "CONTRAST": [0.8, 1.2], "SATURATION": [0.8, 1.2]}
    assert _mapper(cfg, None, 0).jitter is None
    cfg.merge_from_list(["INPUT.COLOR_JITTER.ENABLED", True, "INPUT.COLOR_JITTER.CONTRAST", [0.5, 0.9]])
    add_color_jitter_config(cfg)
    assert color_jitter_args(cfg) == {"enabled": True, "brightness": (0.8, 1.2), "contrast": (0.5, 0.9), "saturation": (0.8, 1.2)}
    assert _mapper(cfg, None, 0).jitter == ((0.8, 1.2), (0.5, 0.9), (0.8, 1.2))
