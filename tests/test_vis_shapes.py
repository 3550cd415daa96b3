"""The drawing names of cubercnn.vis that run on csrc/shapes.hip -- face highlights, `draw_transparent_polygon`, `get_polygon_grid`,
`draw_circle`, `draw_transparent_square`, the ground grid of `draw_scene_view` and demo/demo.py's --ground-grid -- and the host helpers
`interp_color`, `create_colorbar`, `imhstack`, `imvstack`.  The kernels are pinned in test_fill_shapes.py / test_ground_grid.py; here
the rows the Python layer feeds them are checked against float64 evaluations of the reference's formulas written in this file.  The
reference addresses a pixel by its integer coordinates, this repository samples it at (x + 0.5, y + 0.5): the expected masks test
the integer pixel (x, y) against the unshifted vertices, as the reference does.  Pixels within 1e-3 px of an edge or a radius are
left out, at most 0.5 % of the painted ones."""
import argparse
import importlib.util
import json
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import ROOT

TOL, UNSURE_CAP = 1e-3, 0.005
BG, FG = (225, 225, 225), (175, 175, 175)


def _K(H, W):
    return np.array([[1.1 * W, 0.0, 0.5 * W + 0.8], [0.0, 1.1 * W, 0.5 * H - 1.3], [0.0, 0.0, 1.0]])


def _noise(H, W, seed=0):
    return np.random.RandomState(seed).randint(0, 256, size=(H, W, 3)).astype(np.uint8)


def _polygon_mask(H, W, pts):
    """crossing number of the integer pixel (x, y) against the polygon, float64 -> (inside, unsure)"""
    pts = np.asarray(pts, np.float64)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    count, unsure = np.zeros((H, W), np.int64), np.zeros((H, W), bool)
    for k in range(len(pts)):
        a, b = pts[k], pts[(k + 1) % len(pts)]
        e = b - a
        l2 = float(e @ e)
        s = np.clip(((xs - a[0]) * e[0] + (ys - a[1]) * e[1]) / l2, 0.0, 1.0) if l2 > 0 else np.zeros_like(xs)
        unsure |= np.hypot(xs - a[0] - s * e[0], ys - a[1] - s * e[1]) <= TOL
        if a[1] != b[1]:
            count += ((a[1] > ys) != (b[1] > ys)) & (xs < a[0] + (ys - a[1]) * e[0] / e[1])
    return count % 2 == 1, unsure


def _blend(im, mask, blend, color):
    """the reference's im[mask, c] = im[mask, c] * blend + (1 - blend) * color[c], float64 into uint8"""
    out = im.copy()
    for c in range(3):
        out[mask, c] = np.floor(im[mask, c].astype(np.float64) * blend + (1.0 - blend) * color[c]).astype(np.uint8)
    return out


def _box_verts(box, angles):
    from omni3d_amd.cubercnn import util
    return util.mesh_cuboid(box, util.euler2mat(angles)).verts_padded()[0].double().numpy()


# ---- face highlights ----------------------------------------------------------------------------------------------------------------

def test_face_highlights(emu_lib):
    from omni3d_amd.cubercnn import vis
    H, W = 72, 100
    K, color = _K(H, W), (10, 200, 250)
    verts = _box_verts([0.12, 0.07, 3.1, 1.0, 1.2, 1.5], [0.45, 0.52, 0.11])
    edges = vis.draw_3d_box_from_verts(_noise(H, W), K, verts, color=color, thickness=1)
    faces = vis.draw_3d_box_from_verts(_noise(H, W), K, verts, color=color, thickness=1, draw_back=True, draw_top=True)
    proj = (K @ verts.T).T
    proj = proj[:, :2] / proj[:, 2:3]
    back, u_back = _polygon_mask(H, W, proj[[4, 0, 3, 7]])
    top, u_top = _polygon_mask(H, W, proj[[4, 0, 1, 5]])
    unsure = u_back | u_top
    assert back.sum() > 50 and top.sum() > 50 and unsure.sum() <= UNSURE_CAP * (back | top).sum()
    want = _blend(_blend(edges, back, 0.5, color), top, 0.5, color)           # the back face first, then the top face, over the edges
    assert np.array_equal(faces[~unsure], want[~unsure])
    assert np.array_equal(faces[~(back | top) & ~unsure], edges[~(back | top) & ~unsure])          # ... and nowhere else
    assert (faces != edges).any()
    only_back = vis.draw_3d_box_from_verts(_noise(H, W), K, verts, color=color, draw_back=True)
    assert np.array_equal(only_back[~unsure], _blend(edges, back, 0.5, color)[~unsure])
    # a back-face vertex behind the near plane: no back face; the top face (vertices 4, 0, 1, 5) is still drawn
    behind = verts.copy()
    behind[7, 2] = -0.5
    got = vis.draw_3d_box_from_verts(_noise(H, W), K, behind, color=color, draw_back=True, draw_top=True)
    assert np.array_equal(got, vis.draw_3d_box_from_verts(_noise(H, W), K, behind, color=color, draw_top=True))
    assert (got != vis.draw_3d_box_from_verts(_noise(H, W), K, behind, color=color)).any()
    # draw_3d_box hands the two switches on; a device tensor is drawn in place
    from omni3d_amd.cubercnn import util
    R = util.euler2mat([0.45, 0.52, 0.11])
    a = vis.draw_3d_box(_noise(H, W), K, [0.12, 0.07, 3.1, 1.0, 1.2, 1.5], R, color=color, draw_back=True, draw_top=True)
    assert np.array_equal(a, faces)
    dev = torch.from_numpy(np.ascontiguousarray(_noise(H, W).transpose(2, 0, 1)))
    vis.draw_3d_box_from_verts(dev, K, verts, color=color, thickness=1, draw_back=True, draw_top=True)
    assert np.array_equal(dev.numpy().transpose(1, 2, 0), faces)


# ---- polygons, circles, squares ------------------------------------------------------------------------------------------------------

QUAD = np.array([[12.3, 8.7], [61.2, 15.4], [50.8, 52.1], [7.6, 40.9]])
FOLDED = np.array([[12.3, 8.7], [50.8, 52.1], [61.2, 15.4], [7.6, 40.9]])


def test_draw_transparent_polygon_and_polygon_grid(emu_lib):
    from omni3d_amd.cubercnn import vis
    H, W = 60, 75
    for pts in (QUAD, FOLDED):
        inside, unsure = _polygon_mask(H, W, pts)
        assert inside.sum() > 200 and unsure.sum() <= UNSURE_CAP * inside.sum()
        grid = vis.get_polygon_grid(_noise(H, W), pts)
        assert grid.dtype == bool and grid.shape == (H, W) and np.array_equal(grid[~unsure], inside[~unsure])
        for blend in (0.5, 0.25):
            im = _noise(H, W, 2)
            out = vis.draw_transparent_polygon(im, np.concatenate((pts, [[0.0, 0.0]])), blend=blend, color=(0, 255, 255))      # only four rows count
            assert out is im
            want = _blend(_noise(H, W, 2), inside, blend, (0, 255, 255))
            assert np.array_equal(im[~unsure], want[~unsure])
            dev = torch.from_numpy(np.ascontiguousarray(_noise(H, W, 2).transpose(2, 0, 1)))
            assert vis.draw_transparent_polygon(dev, pts, blend=blend, color=(0, 255, 255)) is dev
            assert np.array_equal(dev.numpy().transpose(1, 2, 0), im)         # HWC array and (3,H,W) tensor: the same pixels
    inside, unsure = _polygon_mask(H, W, QUAD[:3])                            # a triangle
    assert np.array_equal(vis.get_polygon_grid(_noise(H, W), QUAD[:3])[~unsure], inside[~unsure])
    with pytest.raises(ValueError):
        vis.get_polygon_grid(_noise(H, W), QUAD[:2])


def test_polygon_grid_agrees_with_matplotlib(emu_lib):
    """the reference's own `get_polygon_grid` (vis.py:540-554): Path(poly_verts).contains_points on the integer pixel grid"""
    mpath = pytest.importorskip("matplotlib.path")
    from omni3d_amd.cubercnn import vis
    H, W = 60, 75
    for pts in (QUAD, FOLDED):
        x, y = np.meshgrid(np.arange(W), np.arange(H))
        want = mpath.Path(pts).contains_points(np.vstack((x.flatten(), y.flatten())).T).reshape(H, W)
        _, unsure = _polygon_mask(H, W, pts)
        got = vis.get_polygon_grid(np.zeros((H, W, 3), np.uint8), pts)
        assert want.sum() > 200 and np.array_equal(got[~unsure], want[~unsure])


def test_draw_circle(emu_lib):
    from omni3d_amd.cubercnn import vis
    H, W = 50, 64
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    for pos, radius, thickness, fill in (((30.7, 21.2), 9, 1, True), ((30.7, 21.2), 9, 1, False), ((30.7, 21.2), 12, 3, False),
                                         ((60.2, 3.9), 7, 1, True), ((12.4, 40.8), 0, 1, True)):
        dist = np.hypot(xs - int(pos[0]), ys - int(pos[1]))                   # integer pixels around the integer centre, as cv2.circle
        outer, inner = (radius + 0.5, 0.0) if fill else (radius + thickness / 2, radius - thickness / 2)
        inside = (dist <= outer) & (dist >= inner)
        unsure = (np.abs(dist - outer) <= TOL) | ((inner > 0) & (np.abs(dist - inner) <= TOL))
        assert unsure.sum() <= UNSURE_CAP * inside.sum() and inside.any()
        im = _noise(H, W, 3)
        vis.draw_circle(im, pos, radius=radius, thickness=thickness, color=(250, 100, 100), fill=fill)
        want = _noise(H, W, 3)
        want[inside] = (250, 100, 100)
        assert np.array_equal(im[~unsure], want[~unsure]), (pos, radius, fill)
        if radius == 0:
            assert inside.sum() == 1                                          # the one pixel, as OpenCV paints it


def test_draw_transparent_square(emu_lib):
    from omni3d_amd.cubercnn import vis
    H, W = 40, 56
    for pos, alpha, radius in (((20.6, 15.3), 0.5, 5), ((3.2, 37.9), 0.25, 6), ((54.9, 2.1), 0.0, 4.5), ((20.6, 15.3), 1, 5)):
        # vis.py:686-702 by hand: rows from pos[1], columns from pos[0], floor, clipped to the image, both ends included
        l, r = (int(np.clip(np.floor(v), 0, H)) for v in (pos[1] - radius, pos[1] + radius))
        t, b = (int(np.clip(np.floor(v), 0, W)) for v in (pos[0] - radius, pos[0] + radius))
        mask = np.zeros((H, W), bool)
        mask[l:r + 1, t:b + 1] = True
        im = _noise(H, W, 4)
        vis.draw_transparent_square(im, pos, alpha=alpha, radius=radius, color=(250, 100, 100))
        assert np.array_equal(im, _blend(_noise(H, W, 4), mask, alpha, (250, 100, 100))), (pos, alpha)
    im = _noise(H, W, 4)
    vis.draw_transparent_square(im, (-30.0, -30.0), alpha=0.0, radius=5)      # every bound negative: nothing, as in the reference
    assert np.array_equal(im, _noise(H, W, 4))


# ---- host helpers --------------------------------------------------------------------------------------------------------------------

def test_host_helpers():
    from omni3d_amd.cubercnn import vis
    assert vis.interp_color(0.25) == (0.0, 62.5, 250.0)
    assert vis.interp_color(3.0, [1, 5], (10, 20, 30), (50, 0, 130)) == (30.0, 10.0, 80.0)
    bar = vis.create_colorbar(4, 3)
    assert bar.shape == (4, 3, 3) and bar.dtype == np.uint8
    # row h: the colour at (h + 0.5) / 4 on the way from color_hi (top) to color_lo: g = 250 * (1 - (h + 0.5) / 4), truncated
    assert bar[:, :, 1].tolist() == [[218] * 3, [156] * 3, [93] * 3, [31] * 3] and (bar[:, :, 0] == 0).all() and (bar[:, :, 2] == 250).all()
    a, b = _noise(40, 30, 5), _noise(20, 50, 6)
    # imhstack: sf = 40 / 20 = 2 > 1: the second image becomes 40 high and int(50 / 2) = 25 wide
    h = vis.imhstack(a, b)
    assert h.shape == (40, 30 + 25, 3) and h.dtype == np.uint8 and np.array_equal(h[:, :30], a)
    h = vis.imhstack(b, a)                                                    # sf = 0.5 < 1: the first becomes 40 high, int(50 / 0.5) = 100 wide
    assert h.shape == (40, 100 + 30, 3) and np.array_equal(h[:, 100:], a)
    assert np.array_equal(vis.imhstack(a, a), np.hstack((a, a)))
    # imvstack: sf = 30 / 50 < 1: the first image becomes 50 wide and int(40 / 0.6) = 66 high
    v = vis.imvstack(a, b)
    assert v.shape == (66 + 20, 50, 3) and np.array_equal(v[66:], b)
    v = vis.imvstack(b, a)                                                    # sf = 50 / 30 > 1: the second becomes 50 wide, int(40 / (5 / 3)) = 24 high
    assert v.shape == (20 + 24, 50, 3) and np.array_equal(v[:20], b)
    flat = np.full((40, 30, 3), 77, np.uint8)
    assert (vis.imvstack(flat, b)[:66] == 77).all()                           # resizing a flat image keeps it flat


# ---- the ground grid of the novel view ---------------------------------------------------------------------------------------------

def _two_boxes():
    from omni3d_amd.cubercnn import util
    far = util.mesh_cuboid([0.0, 0.2, 4.0, 1.0, 1.0, 1.6], util.euler2mat([0.0, 0.4, 0.0]), color=[0.2, 0.6, 0.4])
    near = util.mesh_cuboid([0.3, -0.35, 2.6, 0.8, 0.9, 1.0], util.euler2mat([0.0, -0.3, 0.0]), color=[0.7, 0.3, 0.1])
    return [near, far]


def _is_color(a, color):
    return (a == np.array(color, np.uint8)).all(-1)


def _run_ground(dev):
    from omni3d_amd.cubercnn import vis
    from omni3d_amd.kernels import render
    H, W, scale = 96, 128, 200
    K, im, meshes = _K(H, W), _noise(H, W, 7), _two_boxes()
    plain, white = vis.draw_scene_view(im, K, meshes, mode="novel", scale=scale)
    off, white2 = vis.draw_scene_view(im, K, meshes, mode="novel", scale=scale, ground_grid=False)
    assert (white == 255).all() and (white2 == 255).all() and np.array_equal(plain, off)          # the default call draws no grid
    calls = []
    launch = render.ground_grid
    try:
        render.ground_grid = lambda *a, **k: (calls.append(1), launch(*a, **k))[1]
        view, canvas = vis.draw_scene_view(im, K, meshes, mode="novel", scale=scale, ground_grid=True)
        assert len(calls) == 2                                                # the canvas, and the view under the mask
        again, canvas2 = vis.draw_scene_view(im, K, meshes, mode="novel", scale=scale, canvas=canvas)
        assert len(calls) == 2                                                # a canvas handed in: no grid launch
    finally:
        render.ground_grid = launch
    assert canvas.shape == (scale, scale, 3) and canvas.dtype == np.uint8
    line, ground = _is_color(canvas, FG), _is_color(canvas, BG)
    assert (line | ground).all() and 0.02 * scale * scale < line.sum() < 0.5 * scale * scale      # only the two grid colours, both there
    drawn = (plain != 255).any(-1)                                            # where the call without a grid put a box or an edge
    assert drawn.sum() > 0.02 * scale * scale
    assert np.array_equal(view[~drawn], canvas[~drawn]) and np.array_equal(view[drawn], plain[drawn])
    assert np.array_equal(again, view) and np.array_equal(canvas2, canvas)
    f3, n3, c3 = vis.draw_scene_view(im, K, meshes, mode="front_and_novel", scale=scale, ground_grid=True)
    assert np.array_equal(n3, view) and np.array_equal(c3, canvas) and np.array_equal(f3, vis.draw_scene_view(im, K, meshes, mode="front"))
    # ground_bounds: the plane at y = 0.7 (the scene's largest y) with lines X = -1 .. 0 and Z = 2 .. 4 only
    _, small = vis.draw_scene_view(im, K, meshes, mode="novel", scale=scale, ground_bounds=(0.7, -1, 2, 2, 6))
    few = _is_color(small, FG)
    assert (few | _is_color(small, BG)).all() and 0 < few.sum() < line.sum()
    assert not (few & ~line).any()                                            # the same plane and whole-number lines: a subset of the full grid
    assert not few[0].any() and not few[-1].any() and not few[:, 0].any() and not few[:, -1].any()
    # a plane that lies behind the viewer everywhere: the invalid scene of the reference
    from omni3d_amd.cubercnn.vis import vis as V
    Kn = K.copy()
    assert V._ground_in_view(Kn, np.eye(3), np.zeros(3), (1.0, -5, 5, 1, 9), scale)
    assert not V._ground_in_view(Kn, np.eye(3), np.zeros(3), (1.0, -5, 5, -9, -1), scale)          # behind the camera
    assert not V._ground_in_view(Kn, np.eye(3), np.zeros(3), (1.0, 400, 500, 1, 9), scale)         # far off to the right
    with pytest.raises(ValueError):
        vis.draw_scene_view(im, K, meshes, mode="novel", scale=scale, canvas=np.zeros((scale, scale + 1, 3), np.uint8))


def test_ground_grid_of_the_novel_view_emulated(emu_lib):
    _run_ground("cpu")


@pytest.mark.gpu
def test_ground_grid_of_the_novel_view_gpu(hip_lib):
    _run_ground("cuda")


# ---- demo/demo.py --ground-grid -----------------------------------------------------------------------------------------------------

def test_demo_ground_grid_flag(emu_lib, tmp_path):
    from PIL import Image
    from oracle import make_golden as MG
    from test_vis_demo import _FixedDetections, _image
    spec = importlib.util.spec_from_file_location("omni3d_demo_grid", os.path.join(ROOT, "demo", "demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    assert demo.argument_parser().parse_args(["--input-folder", "x", "--ground-grid"]).ground_grid is True
    assert demo.argument_parser().parse_args(["--input-folder", "x"]).ground_grid is False
    folder, cfg_dir = tmp_path / "images", tmp_path / "cfg"
    folder.mkdir()
    cfg_dir.mkdir()
    Image.fromarray(_image(96, 128, 3)).save(str(folder / "wide.png"))
    shutil.copy(os.path.join(ROOT, "configs", "cubercnn_DLA34_FPN.yaml"), str(cfg_dir))
    with open(str(cfg_dir / "category_meta.json"), "w") as f:
        json.dump({"thing_classes": ["cat%02d" % i for i in range(50)]}, f)
    corners = {}
    for flag in (False, True):
        out = tmp_path / ("grid" if flag else "plain")
        cfg = MG.product_cfg(MG.TINY["overrides"] + ["OUTPUT_DIR", str(out), "INPUT.MIN_SIZE_TEST", 64, "INPUT.MAX_SIZE_TEST", 96])
        args = argparse.Namespace(config_file=str(cfg_dir / "cubercnn_DLA34_FPN.yaml"), input_folder=str(folder), focal_length=0,
                                  principal_point=[], threshold=-1.0, display=False, ground_grid=flag, opts=[])
        with torch.no_grad():
            demo.do_test(args, cfg, _FixedDetections("cpu"))
        with Image.open(str(out / "wide_novel.jpg")) as im:
            novel = np.asarray(im.convert("RGB")).astype(np.int64)
        corners[flag] = [novel[y, x] for y in (0, -1) for x in (0, -1)]
    assert all((c > 245).all() for c in corners[False])                       # white, up to the JPEG
    for c in corners[True]:                                                   # one of the two greys, up to the JPEG
        assert (np.abs(c - 225).max() <= 12 or np.abs(c - 175).max() <= 12) and c.max() - c.min() <= 6, c
