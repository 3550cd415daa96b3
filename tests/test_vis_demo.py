"""cubercnn.vis (draw_3d_box_from_verts, draw_scene_view) and demo/demo.py:do_test on csrc/render.hip.  The kernels themselves are
pinned in test_render.py; here the geometry the Python layer feeds them is checked against float64 projections computed in this
file: which pixels an edge may touch (thickness / 2 + 1 px around the projected, near-plane-clipped edge), the paint order, the
novel view's framing, the blends, and the demo's files."""
import argparse
import json
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import ROOT

EDGES = [[0, 1], [1, 2], [2, 3], [3, 0], [1, 5], [5, 6], [6, 2], [4, 5], [4, 7], [6, 7], [0, 4], [3, 7]]
ZPLANE = 0.05


def _K(H, W):
    return np.array([[1.1 * W, 0.0, 0.5 * W + 0.8], [0.0, 1.1 * W, 0.5 * H - 1.3], [0.0, 0.0, 1.0]])


def _clipped_edges(K, verts, zplane=ZPLANE):
    """float64: the part of every edge at depth >= zplane, projected -> list of ((x0, y0), (x1, y1))"""
    out = []
    for i, j in EDGES:
        a, b = verts[i].astype(np.float64), verts[j].astype(np.float64)
        if a[2] < zplane and b[2] < zplane:
            continue
        if a[2] < zplane:
            a = a + (zplane - a[2]) / (b[2] - a[2]) * (b - a)
        elif b[2] < zplane:
            b = a + (zplane - a[2]) / (b[2] - a[2]) * (b - a)
        pa, pb = K @ a / a[2], K @ b / b[2]
        out.append((pa[:2], pb[:2]))
    return out


def _distance(H, W, segs):
    """(H,W) distance of every pixel centre to the nearest of the segments"""
    ys, xs = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    best = np.full((H, W), np.inf)
    for a, b in segs:
        e = b - a
        l2 = float(e @ e)
        s = np.clip(((xs - a[0]) * e[0] + (ys - a[1]) * e[1]) / l2, 0, 1) if l2 > 0 else np.zeros_like(xs)
        best = np.minimum(best, np.hypot(xs - a[0] - s * e[0], ys - a[1] - s * e[1]))
    return best


def _verts(box, R=None):
    from omni3d_amd.cubercnn.util import mesh_cuboid
    return mesh_cuboid(box, R).verts_padded()[0].double().numpy()


def _image(H, W, seed=0):
    """smooth, so that a JPEG round trip stays close"""
    ys, xs = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    rs = np.random.RandomState(seed)
    ch = [90 + 60 * np.sin(2 * np.pi * (rs.uniform(0.3, 1.2) * xs + rs.uniform(0.3, 1.2) * ys) + rs.uniform(0, 6)) for _ in range(3)]
    return np.clip(np.rint(np.stack(ch, axis=-1)), 0, 255).astype(np.uint8)


def _run_box_edges(dev):
    from omni3d_amd.cubercnn import util, vis
    H, W = 72, 100
    K = _K(H, W)
    color = (10, 200, 250)
    for thickness in (1, 3):
        for box, ang in (([0.1, 0.0, 3.0, 1.0, 1.2, 1.5], 0.5),          # all in front of the camera
                         ([0.15, 0.05, 0.45, 1.0, 0.3, 0.4], 0.3)):       # width 1 around z = 0.45: some edges cross the near plane, some lie behind it
            verts = _verts(box, util.euler2mat([0.2, ang, 0.1]))
            assert ang != 0.3 or ((verts[:, 2] < ZPLANE).sum() >= 2 and (verts[:, 2] >= ZPLANE).sum() >= 2)
            im = _image(H, W)
            before = im.copy()
            vis.draw_3d_box_from_verts(im, K, verts, color=color, thickness=thickness, zplane=ZPLANE)
            changed = (im != before).any(-1)
            dist = _distance(H, W, _clipped_edges(K, verts))
            assert changed.any()
            assert (dist[changed] <= thickness / 2 + 1).all(), float(dist[changed].max())
            assert changed[dist <= thickness / 2 - 1e-3].all()           # ... and the whole clipped edge is there, up to its end points
            assert (im[changed] == np.array(color, np.uint8)).all()
    # a box wholly behind the near plane draws nothing
    im = _image(H, W)
    before = im.copy()
    vis.draw_3d_box_from_verts(im, K, _verts([0.0, 0.0, -2.0, 1.0, 1.0, 1.0]), color=color, thickness=2)
    assert np.array_equal(im, before)
    # an edge that crosses the near plane ends at the projected intersection, whichever end is behind
    v = np.zeros((8, 3))
    v[:, 2] = -1.0
    v[0], v[1] = [0.2, 0.1, 1.0], [-0.1, 0.05, -0.5]
    for a, b in ((0, 1), (1, 0)):
        vv = v.copy()
        vv[0], vv[1] = v[a], v[b]
        rows = [r for r in vis.vis.box_segments(K, vv, color, 2, ZPLANE)]
        assert len(rows) == 3                                          # edges 0-1, 3-0 and 0-4 / 1-2, 0-1 and 1-5 reach the front vertex
        hit = v[0] + (ZPLANE - 1.0) / (-0.5 - 1.0) * (v[1] - v[0])
        want = (K @ hit / hit[2])[:2]
        ends = [np.array(r[0:2]) for r in rows] + [np.array(r[2:4]) for r in rows]
        assert min(np.abs(e - want).max() for e in ends) < 1e-9


def test_draw_3d_box_from_verts_emulated(emu_lib):
    _run_box_edges("cpu")


@pytest.mark.gpu
def test_draw_3d_box_from_verts_gpu(hip_lib):
    _run_box_edges("cuda")


def _two_boxes():
    from omni3d_amd.cubercnn import util
    far = util.mesh_cuboid([0.0, 0.2, 4.0, 1.0, 1.0, 1.6], util.euler2mat([0.0, 0.4, 0.0]), color=[0.2, 0.6, 0.4])
    near = util.mesh_cuboid([0.3, -0.35, 2.6, 0.8, 0.9, 1.0], util.euler2mat([0.0, -0.3, 0.0]), color=[0.7, 0.3, 0.1])
    return [near, far]          # the reference paints in descending mean y of the vertices (vis.py:289): `near`, above `far`, comes last


def _edge_color(mesh):
    return np.array([min(255.0, c * 255 * 1.25) for c in mesh.color[0].tolist()])


def _run_scene_view(dev):
    from omni3d_amd.cubercnn import vis
    H, W, scale = 96, 128, 400
    K = _K(H, W)
    im = _image(H, W, 1)
    meshes = _two_boxes()
    thickness = max(2, int(np.round(3 * H / 1250)))
    # shapes and dtypes per mode
    out2d = vis.draw_scene_view(im, K, meshes, mode="2D_only")
    front = vis.draw_scene_view(im, K, meshes, mode="front")
    novel, canvas = vis.draw_scene_view(im, K, meshes, mode="novel", scale=scale)
    f2, n2, c2 = vis.draw_scene_view(im, K, meshes, mode="front_and_novel", scale=scale, text=["a 0.90", "b 0.80"])
    for a in (out2d, front, f2):
        assert a.shape == (H, W, 3) and a.dtype == np.uint8
    for a in (novel, canvas, n2, c2):
        assert a.shape == (scale, scale, 3) and a.dtype == np.uint8
    assert (canvas == 255).all() and (out2d != im).any() and (front != im).any()
    with pytest.raises(ValueError):
        vis.draw_scene_view(im, K, meshes, mode="side")
    # 'front' without the shaded overlay touches only the neighbourhood of the projected edges
    lines = vis.draw_scene_view(im, K, meshes, mode="front", blend_weight=0.0)
    verts = [m.verts_padded()[0].double().numpy() for m in meshes]
    dist = [_distance(H, W, _clipped_edges(K, v)) for v in verts]
    changed = (lines != im).any(-1)
    assert changed.any() and (np.minimum(dist[0], dist[1])[changed] <= thickness / 2 + 1).all()
    # where edges of both boxes pass, the nearer (later painted) box wins
    both = (dist[0] <= thickness / 2 - 0.25) & (dist[1] <= thickness / 2 - 0.25)
    assert both.sum() >= 4
    assert (lines[both] == np.rint(_edge_color(meshes[0])).astype(np.uint8)).all()
    only_far = (dist[1] <= thickness / 2 - 0.25) & (dist[0] > thickness / 2 + 0.25)
    assert only_far.any() and (lines[only_far] == np.rint(_edge_color(meshes[1])).astype(np.uint8)).all()
    # with the overlay, pixels inside a box and away from the edges move towards the box colour and nothing else moves
    away = np.minimum(dist[0], dist[1]) > thickness / 2 + 1
    assert ((front != im).any(-1) & away).any()
    # the novel view: every box is in it and the drawing stays clear of the margin the zoom search keeps (the vertices stay 1 % of
    # `scale` inside the canvas; an edge reaches thickness / 2 beyond them)
    inked = (novel != 255).any(-1)
    t_novel = max(2, int(np.round(3 * scale / 1250)))
    band = int(np.floor(scale * 0.01 - t_novel / 2))
    assert band >= 2
    assert not inked[:band].any() and not inked[-band:].any() and not inked[:, :band].any() and not inked[:, -band:].any()
    for m in meshes:
        assert (novel == np.rint(_edge_color(m)).astype(np.uint8)).all(-1).sum() > 20
    assert inked.sum() > 0.02 * scale * scale                             # shaded faces, not just lines
    # blend_weight_overlay: 0.85 x the full drawing + 0.15 x the input
    mixed = vis.draw_scene_view(im, K, meshes, mode="front", blend_weight_overlay=0.85)
    want = 0.85 * front.astype(np.float64) + 0.15 * im.astype(np.float64)
    assert np.abs(mixed.astype(np.float64) - want).max() <= 1.0


def test_draw_scene_view_emulated(emu_lib):
    _run_scene_view("cpu")


@pytest.mark.gpu
def test_draw_scene_view_gpu(hip_lib):
    _run_scene_view("cuda")


# ---- demo/demo.py ---------------------------------------------------------------------------------------------------------------

class _Recorder(torch.nn.Module):
    """the model, remembering what it returned"""

    def __init__(self, model):
        super().__init__()
        self.model, self.seen = model, []

    def forward(self, batched):
        out = self.model(batched)
        self.seen.append(out[0]["instances"])
        return out


class _FixedDetections(torch.nn.Module):
    """Stand-in for the detector in the host-emulated case: one forward of even the smallest model takes about 40 s per image under
    the emulator, so there `do_test` is driven with detections made up from the input's size; the GPU case runs the real model."""

    def __init__(self, dev):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1, device=dev))

    def forward(self, batched):
        from omni3d_amd.cubercnn.util import euler2mat, mesh_cuboid
        from omni3d_amd.d2.structures import Instances
        b = batched[0]
        assert b["image"].dtype == torch.uint8 and b["image"].shape[0] == 3 and b["image"].device == self.anchor.device
        assert min(b["image"].shape[1:]) == 64                             # the test-time resize has run
        g = torch.Generator().manual_seed(int(b["height"]))
        n = 5
        inst = Instances((b["height"], b["width"]))
        inst.scores = torch.linspace(0.9, 0.1, n)
        inst.pred_classes = torch.randint(0, 50, (n,), generator=g)
        z = 3.0 + 4.0 * torch.rand(n, generator=g)
        inst.pred_center_cam = torch.stack(((torch.rand(n, generator=g) - 0.5) * 0.4 * z, (torch.rand(n, generator=g) - 0.5) * 0.3 * z, z), 1)
        inst.pred_dimensions = 0.4 + torch.rand(n, 3, generator=g)
        inst.pred_pose = torch.stack([torch.tensor(euler2mat([0.1 * i, 0.7 * i, 0.0]), dtype=torch.float32) for i in range(n)])
        inst.pred_bbox3D = mesh_cuboid(torch.cat((inst.pred_center_cam, inst.pred_dimensions), 1), inst.pred_pose).verts_padded()
        return [{"instances": inst}]


def _run_demo(dev, tmp_path, real_model):
    import importlib.util
    from PIL import Image
    from oracle import make_golden as MG
    from omni3d_amd import synthetic
    spec = importlib.util.spec_from_file_location("omni3d_demo", os.path.join(ROOT, "demo", "demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    folder, cfg_dir = tmp_path / "images", tmp_path / "cfg"
    folder.mkdir()
    cfg_dir.mkdir()
    sizes = {"wide": (96, 128), "tall": (128, 96)}
    for i, (name, (h, w)) in enumerate(sizes.items()):
        Image.fromarray(_image(h, w, 3 + i)).save(str(folder / (name + ".png")))
    shutil.copy(os.path.join(ROOT, "configs", "cubercnn_DLA34_FPN.yaml"), str(cfg_dir))
    cats = ["cat%02d" % i for i in range(50)]
    with open(str(cfg_dir / "category_meta.json"), "w") as f:
        json.dump({"thing_classes": cats}, f)
    spec_t = MG.TINY
    priors = synthetic.make_priors(50)

    def run(threshold, out):
        cfg = MG.product_cfg(spec_t["overrides"] + ["OUTPUT_DIR", str(out), "INPUT.MIN_SIZE_TEST", 64, "INPUT.MAX_SIZE_TEST", 96,
                                                    "MODEL.RPN.PRE_NMS_TOPK_TEST", 100, "MODEL.RPN.POST_NMS_TOPK_TEST", 30, "TEST.DETECTIONS_PER_IMAGE", 12])
        model = _Recorder(MG.build_product_model(cfg, priors, spec_t["seed"], device=dev) if real_model else _FixedDetections(dev))
        args = argparse.Namespace(config_file=str(cfg_dir / "cubercnn_DLA34_FPN.yaml"), input_folder=str(folder), focal_length=0,
                                  principal_point=[], threshold=threshold, display=True, opts=[])
        with torch.no_grad():
            demo.do_test(args, cfg, model)
        return model.seen

    out = tmp_path / "all"
    seen = run(-1.0, out)
    assert len(seen) == 2
    for inst, name in zip(seen, sorted(sizes)):                        # list_files sorts: tall, wide
        h, w = sizes[name]
        assert len(inst) > 0
        for suffix, shape in (("_boxes.jpg", (h, w)), ("_novel.jpg", (h, h))):
            with Image.open(str(out / (name + suffix))) as im:
                assert im.size == (shape[1], shape[0])
        rows = json.load(open(str(out / (name + ".json"))))
        assert len(rows) == len(inst)
        for k, row in enumerate(rows):
            assert row["category"] == cats[int(inst.pred_classes[k])] and row["score"] == float(inst.scores[k])
            assert row["center_cam"] == inst.pred_center_cam[k].tolist() and row["dimensions"] == inst.pred_dimensions[k].tolist()
            assert row["pose"] == inst.pred_pose[k].tolist() and row["bbox3D"] == inst.pred_bbox3D[k].tolist()
    # nothing above the threshold: the untouched image as <name>_boxes.jpg and an empty detection list, nothing else
    out = tmp_path / "none"
    run(2.0, out)
    assert sorted(os.listdir(str(out))) == ["tall.json", "tall_boxes.jpg", "wide.json", "wide_boxes.jpg"]
    for name in sizes:
        assert json.load(open(str(out / (name + ".json")))) == []
        with Image.open(str(out / (name + "_boxes.jpg"))) as im:
            got = np.asarray(im.convert("RGB")).astype(np.float64)
        with Image.open(str(folder / (name + ".png"))) as im:
            src = np.asarray(im.convert("RGB")).astype(np.float64)
        # JPEG at PIL's default quality on a smooth image: a few grey levels (8 x 8 DCT quantisation + chroma subsampling)
        assert np.abs(got - src).mean() < 2.0 and np.abs(got - src).max() < 16.0


def test_demo_do_test_emulated(emu_lib, tmp_path):
    _run_demo("cpu", tmp_path, real_model=False)


@pytest.mark.gpu
def test_demo_do_test_gpu(hip_lib, tmp_path):
    _run_demo("cuda", tmp_path, real_model=True)
