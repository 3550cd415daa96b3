"""Drawing predicted 3D boxes (reference cubercnn/vis/vis.py:210-383, 571-651) on csrc/render.hip: the shaded overlay is a ray cast
against the cuboids (`omni_cuboid_depth` + `omni_scene_compose`) instead of pytorch3d's mesh renderer, the box edges are thick
segments painted by `omni_draw_segments` instead of `cv2.line`, blended faces, circles and squares are `omni_fill_shapes` rows
(csrc/shapes.hip) and the ground of the novel view is `omni_ground_grid`.  Images enter and leave as the reference's numpy HWC uint8 arrays;
in between they live on the device as (3,H,W) tensors.  Labels are written last, on the host, with PIL's built-in bitmap font (a
stated departure from OpenCV's Hershey font; not on the hot path).
`visualize_from_instances` (vis.py:76-196), the last step of every evaluation: the per-dataset 3D error line from one launch of
csrc/vis_errors.hip (`match_errors_from_instances`) and a drawing of every 50th image."""
import os
from copy import deepcopy

import numpy as np
import torch

from ...d2.structures import BoxMode
from ...kernels import render, viserr
from ..util import math_util as MU
from ..util import util as U

# the twelve edges in the reference's drawing order (vis.py:593)
BOX_EDGES = [[0, 1], [1, 2], [2, 3], [3, 0], [1, 5], [5, 6], [6, 2], [4, 5], [4, 7], [6, 7], [0, 4], [3, 7]]


def _to_device(im):
    """numpy HWC uint8 -> contiguous (3,H,W) uint8 tensor on the drawing device"""
    chw = np.ascontiguousarray(np.asarray(im).astype(np.uint8, copy=False).transpose(2, 0, 1))
    return torch.from_numpy(chw).to(render.default_device())


def _to_host(t):
    return np.ascontiguousarray(t.cpu().numpy().transpose(1, 2, 0))


def box_segments(K, verts3d, color, thickness, zplane=0.05, eps=1e-4):
    """The visible part of the twelve edges of one box as rows [x0, y0, x1, y1, thickness, c0, c1, c2], with the near-plane rule of
    vis.py:599-619: an edge with both ends in front of `zplane` is dropped, one that crosses it ends at the intersection.  End
    points stay at sub-pixel precision (the reference truncates them to integers for cv2.line)."""
    K = np.asarray(K.detach().cpu().numpy() if isinstance(K, torch.Tensor) else K, dtype=np.float64)
    verts3d = np.asarray(verts3d.detach().cpu().numpy() if isinstance(verts3d, torch.Tensor) else verts3d, dtype=np.float64)
    rows = []
    for i, j in BOX_EDGES:
        v0, v1 = verts3d[i], verts3d[j]
        z0, z1 = v0[-1], v1[-1]
        if z0 >= zplane or z1 >= zplane:
            if (z0 < zplane) != (z1 < zplane):
                # intersection of the edge with the near plane.  (The reference divides by max(z1 - z0, eps), which is eps for an
                # edge that runs towards the camera; the intersection itself is what it means.)
                new_v = v0 + (zplane - z0) / (z1 - z0) * (v1 - v0)
                if z0 < zplane:
                    v0 = new_v
                else:
                    v1 = new_v
            p0, p1 = (K @ v0) / max(v0[-1], eps), (K @ v1) / max(v1[-1], eps)
            rows.append([p0[0], p0[1], p1[0], p1[1], float(thickness), float(color[0]), float(color[1]), float(color[2])])
    return rows


def _paint(image, rows, shapes=()):
    """segment rows, then shape rows (omni_fill_shapes), onto the device image"""
    if rows:
        render.draw_segments(image, torch.tensor(rows, dtype=torch.float32).to(image.device))
    if shapes:
        render.fill_shapes(image, torch.tensor(shapes, dtype=torch.float32).to(image.device))


def _draw_rows(im, rows, shapes=()):
    """segment rows and then shape rows onto `im`, in place: numpy HWC uint8 (through the device and back, once) or a (3,H,W) uint8
    tensor on the device"""
    if isinstance(im, torch.Tensor):
        _paint(im, rows, shapes)
        return im
    dev = _to_device(im)
    _paint(dev, rows, shapes)
    im[...] = _to_host(dev)
    return im


def _height_width(im):
    return tuple(im.shape[1:]) if isinstance(im, torch.Tensor) else tuple(im.shape[:2])


def _quad_row(verts, blend, color):
    """four (x, y) vertices in the reference's coordinates, where an integer names a pixel: that pixel's centre is (x + 0.5, y + 0.5)
    in the coordinates of omni_fill_shapes, so the vertices move by half a pixel"""
    v = np.asarray(verts.detach().cpu().numpy() if isinstance(verts, torch.Tensor) else verts, dtype=np.float64)[:4, :2]
    if v.shape[0] == 3:
        v = np.concatenate((v, v[-1:]))                  # a triangle: the fourth edge has no length and is never crossed
    if v.shape != (4, 2):
        raise ValueError("a polygon of three or four (x, y) vertices is needed, got {}".format(v.shape))
    return [0.0] + (v + 0.5).reshape(8).tolist() + [float(blend), float(color[0]), float(color[1]), float(color[2])]


def get_polygon_grid(im, poly_verts):
    """vis.py:540-554: bool (H,W), true where the pixel (x, y) lies inside the polygon `poly_verts` (three or four vertices, even-odd
    rule).  Only the size of `im` (numpy HWC or a (3,H,W) tensor) is used.  The reference asks matplotlib's `Path.contains_points`."""
    H, W = _height_width(im)
    mask = torch.zeros((3, H, W), dtype=torch.uint8, device=render.default_device())
    _paint(mask, [], [_quad_row(poly_verts, 0.0, (255, 255, 255))])
    return mask[0].cpu().numpy() > 0


def draw_transparent_polygon(im, verts, blend=0.5, color=(0, 255, 255)):
    """vis.py:562-568: every pixel inside the polygon of the first four rows of `verts` becomes floor(v * blend + (1 - blend) * color)
    (the reference's float64 expression stored into uint8; `blend` is carried as float32), in place"""
    return _draw_rows(im, [], [_quad_row(verts, blend, color)])


def draw_circle(im, pos, radius=5, thickness=1, color=(250, 100, 100), fill=True):
    """vis.py:556-560 (`cv2.circle`) around the pixel (int(pos[0]), int(pos[1])): filled, every pixel whose centre is within radius +
    0.5 of that pixel's centre (radius 0 paints the one pixel, as OpenCV does); as an outline, those between radius - thickness / 2
    and radius + thickness / 2.  A stated departure: the true disc, not OpenCV's midpoint circle."""
    cx, cy = int(pos[0]) + 0.5, int(pos[1]) + 0.5
    outer, inner = (radius + 0.5, 0.0) if fill else (radius + thickness / 2, max(radius - thickness / 2, 0.0))
    return _draw_rows(im, [], [[1.0, cx, cy, float(outer), float(inner), 0.0, 0.0, 0.0, 0.0, 0.0, float(color[0]), float(color[1]), float(color[2])]])


def draw_transparent_square(im, pos, alpha=1, radius=5, color=(250, 100, 100)):
    """vis.py:684-703: the pixels of rows floor(pos[1] - radius) .. floor(pos[1] + radius) and columns floor(pos[0] - radius) ..
    floor(pos[0] + radius), each bound clipped to the image as the reference clips it, become floor(v * alpha + (1 - alpha) * color)"""
    H, W = _height_width(im)
    bounds = np.array([pos[1] - radius, pos[1] + radius, pos[0] - radius, pos[0] + radius], dtype=np.float64)
    if not (bounds >= 0).any():
        return im
    l, r = (int(v) for v in np.clip(np.floor(bounds[:2]), 0, H))
    t, b = (int(v) for v in np.clip(np.floor(bounds[2:]), 0, W))
    # the pixels t .. b of the reference span [t, b + 1] here; the half-pixel shift of _quad_row is already in these numbers
    row = [0.0, t, l, b + 1, l, b + 1, r + 1, t, r + 1, float(alpha), float(color[0]), float(color[1]), float(color[2])]
    return _draw_rows(im, [], [[float(v) for v in row]])


def interp_color(dist, bounds=[0, 1], color_lo=(0, 0, 250), color_hi=(0, 250, 250)):
    """vis.py:17-24: the colour at `dist` on the straight line from color_lo (at bounds[0]) to color_hi (at bounds[1])"""
    w = (dist - bounds[0]) / (bounds[1] - bounds[0])
    return tuple(lo * (1 - w) + hi * w for lo, hi in zip(color_lo[:3], color_hi[:3]))


def create_colorbar(height, width, color_lo=(0, 0, 250), color_hi=(0, 250, 250)):
    """vis.py:62-73: (height, width, 3) uint8, row h in the colour at h + 0.5 of [0, height], color_hi at the top"""
    rows = [interp_color(h + 0.5, [0, height], color_hi, color_lo) for h in range(height)]
    return np.repeat(np.asarray(rows, dtype=np.float64).reshape(height, 1, 3), width, axis=1).astype(np.uint8)


def _resize(im, width, height):
    """bilinear, on the host with PIL (the reference calls cv2.resize)"""
    from PIL import Image
    return np.asarray(Image.fromarray(np.ascontiguousarray(im)).resize((int(width), int(height)), Image.BILINEAR))


def imhstack(im1, im2):
    """vis.py:717-729: side by side; the lower image is first resized to the height of the other and to the reference's width,
    int(width / sf) with sf the ratio of the heights"""
    sf = im1.shape[0] / im2.shape[0]
    if sf > 1:
        im2 = _resize(im2, int(im2.shape[1] / sf), im1.shape[0])
    elif sf < 1:
        im1 = _resize(im1, int(im1.shape[1] / sf), im2.shape[0])
    return np.hstack((im1, im2))


def imvstack(im1, im2):
    """vis.py:732-743: one above the other; the narrower image is first resized to the width of the other and to the reference's
    height, int(height / sf) with sf the ratio of the widths.  (The reference hands these two numbers to cv2.resize in the order
    (height, width), after which np.vstack only works when they happen to agree; here they are used as what they are.)"""
    sf = im1.shape[1] / im2.shape[1]
    if sf > 1:
        im2 = _resize(im2, im1.shape[1], int(im2.shape[0] / sf))
    elif sf < 1:
        im1 = _resize(im1, im2.shape[1], int(im1.shape[0] / sf))
    return np.vstack((im1, im2))


def _cv_segment(v0, v1, color, thickness):
    """one `cv2.line` call as a segment row: the end points are truncated to integers as cv2.line receives them; OpenCV's integer
    (x, y) names a pixel, whose centre is (x + 0.5, y + 0.5) in the coordinates of omni_draw_segments"""
    return [int(v0[0]) + 0.5, int(v0[1]) + 0.5, int(v1[0]) + 0.5, int(v1[1]) + 0.5, float(thickness), float(color[0]), float(color[1]),
            float(color[2])]


def draw_line(im, v0, v1, color=(0, 200, 200), thickness=1):
    """vis.py:58-59: the line from v0 to v1 (x, y), end points truncated to integers, onto `im` in place"""
    return _draw_rows(im, [_cv_segment(v0, v1, color, thickness)])


def draw_2d_box(im, box, color=(0, 200, 200), thickness=1):
    """vis.py:705-714 (`cv2.rectangle`): the outline of box [x, y, w, h] with corners (int(x), int(y)) and (int(x + w - 1),
    int(y + h - 1)), four segments in one launch"""
    x1, y1, x2, y2 = int(box[0]), int(box[1]), int((box[0] + box[2]) - 1), int((box[1] + box[3]) - 1)
    corners = [(x1, y1), (x2, y1), (x2, y2), (x1, y2)]
    return _draw_rows(im, [_cv_segment(corners[k], corners[(k + 1) % 4], color, thickness) for k in range(4)])


def bev_corners(canvas_width, z3d, l3d, w3d, x3d, ry3d, scale=1):
    """the four corners (4,2) of a box in the bird's-eye view of vis.py:26-50, with the reference's swap of w and l"""
    w, l, x, z, r = l3d * scale, w3d * scale, x3d * scale, z3d * scale, ry3d * -1
    corners1 = np.array([[-w / 2, -l / 2, 1], [+w / 2, -l / 2, 1], [+w / 2, +l / 2, 1], [-w / 2, +l / 2, 1]], dtype=np.float64)
    ry = np.array([[+np.cos(r), -np.sin(r), 0], [+np.sin(r), np.cos(r), 0], [0, 0, 1]], dtype=np.float64)
    corners2 = ry.dot(corners1.T).T
    corners2[:, 0] += w / 2 + x + canvas_width / 2
    corners2[:, 1] += l / 2 + z
    return corners2[:, :2]


def draw_bev(canvas_bev, z3d, l3d, w3d, x3d, ry3d, color=(0, 200, 200), scale=1, thickness=2):
    """vis.py:26-55: the footprint of a box on a bird's-eye canvas (HWC uint8 or a device tensor), four segments in one launch.
    -> the corners (4,2) that were joined (the reference returns nothing)"""
    width = canvas_bev.shape[2] if isinstance(canvas_bev, torch.Tensor) else canvas_bev.shape[1]
    c = bev_corners(width, z3d, l3d, w3d, x3d, ry3d, scale)
    _draw_rows(canvas_bev, [_cv_segment(c[k], c[(k + 1) % 4], color, thickness) for k in range(4)])
    return c


BACK_IDXS, TOP_IDXS = [4, 0, 3, 7], [4, 0, 1, 5]          # the highlighted faces (vis.py:596-597)


def face_shapes(K, verts3d, color, zplane=0.05, draw_back=True, draw_top=True):
    """vis.py:628-645 as rows of omni_fill_shapes: the back and / or the top face of the box, blended at 0.5 in `color`; a face with a
    vertex in front of `zplane` is skipped"""
    K = np.asarray(K.detach().cpu().numpy() if isinstance(K, torch.Tensor) else K, dtype=np.float64)
    verts3d = np.asarray(verts3d.detach().cpu().numpy() if isinstance(verts3d, torch.Tensor) else verts3d, dtype=np.float64)
    rows = []
    for wanted, idxs in ((draw_back, BACK_IDXS), (draw_top, TOP_IDXS)):
        v = verts3d[idxs]
        if wanted and np.all(v[:, -1] >= zplane):
            p = (K @ v.T).T
            rows.append(_quad_row(p[:, :2] / p[:, 2:3], 0.5, color))
    return rows


def draw_3d_box_from_verts(im, K, verts3d, color=(0, 200, 200), thickness=1, zplane=0.05, eps=1e-4, *, draw_back=False, draw_top=False):
    """vis.py:571-626: the edges of the box with vertices verts3d (8,3, camera space) onto `im`, in place, then the back face
    (vertices 4, 0, 3, 7) and / or the top face (4, 0, 1, 5) blended over them at 0.5 in the same colour (vis.py:628-645).  im:
    numpy HWC uint8 (as in the reference) or a (3,H,W) uint8 tensor already on the device.  `draw_back` / `draw_top` are keyword-only
    here; the reference has them between `thickness` and `zplane`."""
    shapes = face_shapes(K, verts3d, color, zplane, draw_back, draw_top) if draw_back or draw_top else []
    return _draw_rows(im, box_segments(K, verts3d, color, thickness, zplane, eps), shapes)


def draw_3d_box(im, K, box3d, R, color=(0, 200, 200), thickness=1, view_R=None, view_T=None, *, draw_back=False, draw_top=False):
    """vis.py:648-651: box3d [X,Y,Z,W,H,L] with pose R, optionally seen through the rigid motion (view_R, view_T).  `draw_back` /
    `draw_top` as in `draw_3d_box_from_verts`, keyword-only (the reference has them before `view_R`)."""
    verts = MU.mesh_cuboid(box3d, R).verts_padded()[0].double().numpy()
    if view_R is not None:
        verts = (np.asarray(view_R, dtype=np.float64) @ verts.T).T
    if view_T is not None:
        verts = verts + np.asarray(view_T, dtype=np.float64).reshape(1, 3)
    return draw_3d_box_from_verts(im, K, verts, color=color, thickness=thickness, draw_back=draw_back, draw_top=draw_top)


def draw_text(im, text, pos, scale=0.4, color="auto", bg_color=(0, 255, 255), blend=0.33):
    """vis.py:653-681 on the host with PIL's built-in bitmap font (fixed size: `scale` is accepted and ignored): the label on a
    blended background patch whose lower left corner is `pos`.  im: numpy HWC uint8, in place."""
    from PIL import Image, ImageDraw, ImageFont
    text = str(text)
    font = ImageFont.load_default()
    x0, y0, x1, y1 = font.getbbox(text)
    tw, th = int(x1 - x0), int(y1 - y0)
    H, W = im.shape[:2]
    if color == "auto":
        color = (0, 0, 0) if bg_color is None or (bg_color[0] + bg_color[1] + bg_color[2]) / 3 > 127.5 else (255, 255, 255)
    x_s = int(np.clip(pos[0], 0, W))
    y_e = int(np.clip(pos[1], 0, H))
    y_s = int(np.clip(y_e - th - 4, 0, H))
    x_e = int(np.clip(x_s + tw + 4, 0, W))
    if x_e <= x_s or y_e <= y_s:
        return im
    if bg_color is not None:
        patch = im[y_s:y_e, x_s:x_e].astype(np.float64) * blend + np.asarray(bg_color, dtype=np.float64)[:3] * (1 - blend)
        im[y_s:y_e, x_s:x_e] = np.clip(np.rint(patch), 0, 255).astype(np.uint8)
    pil = Image.fromarray(np.ascontiguousarray(im[y_s:y_e, x_s:x_e]))
    ImageDraw.Draw(pil).text((2 - x0, 2 - y0), text, fill=tuple(int(c) for c in color), font=font)
    im[y_s:y_e, x_s:x_e] = np.asarray(pil)
    return im


def _edge_color(mesh):
    return [min(255.0, float(c) * 255 * 1.25) for c in mesh.color[0].tolist()]


def _paint_order(verts_list):
    """the reference's paint order (vis.py:289, "reverse depth"): descending mean y of the vertices, the smallest mean y last"""
    return list(reversed(np.argsort([float(v[:, 1].mean()) for v in verts_list])))


def _cast(dev, K, box3d, R, color, height, width, zplane):
    """the scene on the device and what every pixel sees of it -> (K, R, color, index, face)"""
    Kt = torch.tensor(np.asarray(K, dtype=np.float32).reshape(9)).to(dev)
    box3d, R, color = box3d.to(dev), R.to(dev), color.to(dev)
    _, index, face, _, _ = render.cuboid_depth(box3d, R, Kt, height, width, zplane)
    return Kt, R, color, index, face


def _shade(image, K, box3d, R, color, blend_weight, zplane):
    Kt, R, color, index, face = _cast(image.device, K, box3d, R, color, image.shape[1], image.shape[2], zplane)
    render.scene_compose(image, index, face, R, Kt, color, blend_weight)
    return index


GROUND_NEAR, GROUND_BG, GROUND_LINE = 0.25, (225, 225, 225), (175, 175, 175)          # vis.py:413, 454-455


def _default_ground_bounds(all_verts):
    """the reference's first estimate (vis.py:392-399): the scene's extent in x and z, widened by 50 extents on either side and
    rounded; the plane lies at the largest y -> (max_y3d, x_start, x_end, z_start, z_end)"""
    lo, hi = all_verts.min(0), all_verts.max(0)
    ex, ez = hi[0] - lo[0], hi[2] - lo[2]
    return (float(hi[1]), int(np.round(lo[0] - ex * 50)), int(np.round(hi[0] + ex * 50)), int(np.round(lo[2] - ez * 50)),
            int(np.round(hi[2] + ez * 50)))


def _ground_in_view(K, A, t, ground_bounds, scale):
    """Is a point of the ground rectangle, at depth >= GROUND_NEAR, projected into [-50, scale + 50) on both image axes?  The
    reference projects a mesh of grid points to find out (vis.py:401-425); here the rectangle is clipped, in view space, against
    the five half-spaces that say so, each linear in the point: something is left or nothing is."""
    y0, x0, x1, z0, z1 = ground_bounds
    poly = [A @ np.array([x, y0, z], dtype=np.float64) + t for x, z in ((x0, z0), (x1 - 1, z0), (x1 - 1, z1 - 1), (x0, z1 - 1))]
    ez = np.array([0.0, 0.0, 1.0])
    planes = [(ez, GROUND_NEAR), (K[0] + 50 * ez, 0.0), ((scale + 50) * ez - K[0], 0.0), (K[1] + 50 * ez, 0.0), ((scale + 50) * ez - K[1], 0.0)]
    for n, d in planes:                                   # Sutherland-Hodgman: keep n . p >= d
        kept = []
        for i, a in enumerate(poly):
            b = poly[(i + 1) % len(poly)]
            fa, fb = float(n @ a) - d, float(n @ b) - d
            if fa >= 0:
                kept.append(a)
            if (fa >= 0) != (fb >= 0):
                kept.append(a + fa / (fa - fb) * (b - a))
        poly = kept
        if not poly:
            return False
    return True


def _ground(image, K, A, t, ground_bounds, scale, index=None):
    """the ground grid of the novel view onto the device image, under the pixels where `index` shows no box"""
    dev = image.device
    f = lambda a: torch.tensor(np.asarray(a, dtype=np.float32).reshape(-1)).to(dev)           # noqa: E731
    return render.ground_grid(image, f(K), f(A), f(t), ground_bounds[0], ground_bounds[1:], index=index, near=GROUND_NEAR,
                              thickness=max(1, int(np.round(3 * scale / 1250))), bg_color=GROUND_BG, line_color=GROUND_LINE)


def _edges_and_labels(image, K, verts_list, meshes, thickness, zplane):
    rows = []
    order = _paint_order(verts_list)
    for m in order:
        rows += box_segments(K, verts_list[m], _edge_color(meshes[m]), thickness, zplane)
    _paint(image, rows)
    return order


def _labels(im, K, verts_list, meshes, text, order):
    if text is None:
        return
    for m in order:
        v = verts_list[m]
        p = (K @ v.T) / v[:, -1]
        draw_text(im, "{}".format(text[m]), [p[0].min(), p[1].min()], scale=0.50 * im.shape[0] / 500, bg_color=_edge_color(meshes[m]))


def draw_scene_view(im, K, meshes, text=None, scale=1000, R=None, T=None, zoom_factor=1.0, mode="front_and_novel", blend_weight=0.80,
                    blend_weight_overlay=1.0, zplane=0.05, ground_bounds=None, canvas=None, ground_grid=False):
    """vis.py:210-538.  im: numpy HWC uint8; K: 3x3; meshes: list of `mesh_cuboid` results (one box each, with a colour); text:
    optional label per mesh.  mode '2D_only' -> image with the 2D boxes of the projected vertices; 'front' -> image with the shaded
    boxes blended in by `blend_weight` (skipped at 0), the box edges painted in the reference's order (descending mean y of the vertices), then the whole drawing blended over the
    input by `blend_weight_overlay`; 'novel' -> (view, canvas): the scene rotated about its centre by R (default euler2mat([pi/3, 0, 0]))
    and zoomed with the reference's search (x0.95 per trial, margin 0.01, stop at z < 0.25; `zoom_factor` is used as given when T is
    set) on a scale x scale canvas; 'front_and_novel' -> (front, view, canvas).  All images are uint8.
    The canvas is white unless `ground_grid` is true or `ground_bounds` = (max_y3d, x3d_start, x3d_end, z3d_start, z3d_end) is given
    (whole numbers; in the reference they come before `zplane`): then it is the ground plane y = max_y3d of the scene with the
    reference's grid of unit squares (vis.py:389-490), painted per pixel by `omni_ground_grid`.  Without `ground_bounds` the bounds are
    the reference's first estimate (`_default_ground_bounds`); if no point of that rectangle projects into [-50, scale + 50) on both
    axes, (im, im, canvas) is returned as in the reference.  A `canvas` from an earlier call (scale x scale x 3) is used as the
    background as it is, without a grid launch.  The returned canvas is the background without the boxes.  On the device: the cast,
    the grid under the pixels that see no box, the shading, the edges; labels on the host.
    Departures from the reference: the renderer is the ray cast of csrc/render.hip (pixel-centre samples, no specular highlight,
    true depth along the ray); grid lines end square at the bounds and at depth 0.25 instead of bending there, keep sub-pixel
    precision and are not drawn above the horizon; the estimated bounds are not narrowed by a second pass (the grid costs the same
    whatever its bounds); labels are written last, on the host."""
    if R is None:
        R = MU.euler2mat([np.pi / 3, 0, 0])
    K = np.asarray(K, dtype=np.float64)
    H, W = im.shape[:2]
    verts_list = [m.verts_padded()[0].double().numpy() for m in meshes]
    thickness = max(2, int(np.round(3 * H / 1250)))

    if mode == "2D_only":
        image = _to_device(im)
        order = _paint_order(verts_list)
        rows, corners = [], {}
        for m in order:
            v = verts_list[m]
            p = (K @ v.T) / v[:, -1]
            x1, y1, x2, y2 = p[0].min(), p[1].min(), p[0].max(), p[1].max()
            corners[m] = (x1, y1)
            c = _edge_color(meshes[m])
            for a, b in (((x1, y1), (x2, y1)), ((x2, y1), (x2, y2)), ((x2, y2), (x1, y2)), ((x1, y2), (x1, y1))):
                rows.append([a[0], a[1], b[0], b[1], float(thickness)] + c)
        _paint(image, rows)
        out = _to_host(image)
        if text is not None:
            for m in order:
                draw_text(out, "{}".format(text[m]), corners[m], scale=0.50 * H / 500, bg_color=_edge_color(meshes[m]))
        return out
    if mode not in ("front", "novel", "front_and_novel"):
        raise ValueError("No visualization written for {}".format(mode))

    box3d = torch.cat([m.box3d for m in meshes])
    Rs = torch.cat([m.R for m in meshes])
    colors = torch.cat([m.color for m in meshes])

    im_drawn_rgb = None
    if mode in ("front_and_novel", "front"):
        image = _to_device(im)
        if blend_weight > 0:
            _shade(image, K, box3d, Rs, colors, blend_weight, zplane)
        order = _edges_and_labels(image, K, verts_list, meshes, thickness, zplane)
        im_drawn_rgb = _to_host(image)
        if 0.0 < blend_weight_overlay < 1.0:       # one pass over the finished drawing, on the host where it is returned
            mix = im_drawn_rgb.astype(np.float64) * blend_weight_overlay + np.asarray(im, dtype=np.float64) * (1 - blend_weight_overlay)
            im_drawn_rgb = np.clip(np.rint(mix), 0, 255).astype(np.uint8)
        _labels(im_drawn_rgb, K, verts_list, meshes, text, order)
        if mode == "front":
            return im_drawn_rgb

    # ---- the novel view (vis.py:315-530) ----
    view_R = np.asarray(R, dtype=np.float64)
    all_verts = np.concatenate(verts_list, axis=0)
    center = (all_verts.min(0) + all_verts.max(0)) / 2 if T is None else np.asarray(T, dtype=np.float64).reshape(3)
    rotated = (view_R @ (all_verts - center).T).T
    K_novel = deepcopy(K)
    K_novel[0, -1] *= scale / W
    K_novel[1, -1] *= scale / H
    margin = 0.01
    if T is None:
        max_trials, zoom_factor = 10000, 100.0
        zoom_in = zoom_factor
        while max_trials:
            zoom_in = zoom_in * 0.95
            v = rotated.copy()
            v[:, -1] += center[-1] * zoom_in
            if (v[:, -1] < 0.25).any():           # zoomed in too much
                break
            proj = (K_novel @ v.T) / v[:, -1]
            if (proj[:2] < scale * margin).any() or (proj[:2] > scale * (1 - margin)).any():
                break
            zoom_factor = zoom_in
            max_trials -= 1
        zoom_out_bias = float(center[-1])
    else:
        zoom_out_bias = 1.0
    shift = np.array([0.0, 0.0, zoom_out_bias * zoom_factor])
    # a rigid motion of the scene: p' = view_R (p - center) + shift, so every box keeps its size, R' = view_R R, c' = view_R (c - center) + shift
    vR = torch.tensor(view_R, dtype=torch.float32)
    box_novel = box3d.clone()
    box_novel[:, :3] = ((box3d[:, :3].double() - torch.tensor(center)) @ torch.tensor(view_R).T + torch.tensor(shift)).float()
    R_novel = vR.unsqueeze(0) @ Rs
    verts_novel = [(view_R @ (v - center).T).T + shift for v in verts_list]
    motion_t = shift - view_R @ center                     # p' = view_R p + motion_t
    if canvas is not None:
        canvas = np.asarray(canvas).astype(np.uint8, copy=False)
        if canvas.shape != (scale, scale, 3):
            raise ValueError("canvas must be {} x {} x 3, got {}".format(scale, scale, canvas.shape))
        ground_bounds = None
    elif ground_grid or ground_bounds is not None:
        if ground_bounds is None:
            ground_bounds = _default_ground_bounds(all_verts)
            if not _ground_in_view(K_novel, view_R, motion_t, ground_bounds, scale):       # invalid scene (vis.py:423-425)
                return im, im, np.full((scale, scale, 3), 255, dtype=np.uint8)
        ground_bounds = (float(ground_bounds[0]),) + tuple(int(np.round(b)) for b in ground_bounds[1:])
    image = _to_device(np.full((scale, scale, 3), 255, dtype=np.uint8) if canvas is None else canvas)
    Kt, R_dev, colors_dev, index, face = _cast(image.device, K_novel, box_novel, R_novel, colors, scale, scale, zplane)
    if ground_bounds is not None:
        canvas = _to_host(_ground(torch.empty_like(image), K_novel, view_R, motion_t, ground_bounds, scale))
        _ground(image, K_novel, view_R, motion_t, ground_bounds, scale, index=index)
    elif canvas is None:
        canvas = np.full((scale, scale, 3), 255, dtype=np.uint8)
    render.scene_compose(image, index, face, R_dev, Kt, colors_dev, 1.0)
    order = _edges_and_labels(image, K_novel, verts_novel, meshes, max(2, int(np.round(3 * scale / 1250))), zplane)
    im_novel_view = _to_host(image)
    _labels(im_novel_view, K_novel, verts_novel, meshes, text, order)
    if mode == "front_and_novel":
        return im_drawn_rgb, im_novel_view, canvas
    return im_novel_view, canvas


# ---- visualize_from_instances (vis.py:76-196) -------------------------------------------------------------------------------------

def _dataset_dicts(dataset):
    """the raw dataset dicts: this package's test loader keeps them as a plain sequence, detectron2's MapDataset as `._dataset`"""
    return getattr(dataset, "_dataset", dataset)


def _pack_instances(detections, dicts):
    """all prediction records and ground-truth annotations as the flat arrays of `viserr.match_errors`, ragged by image"""
    dt_n = [len(o["instances"]) for o in detections]
    gt_n = [len(dicts[i]["annotations"]) for i in range(len(detections))]
    D, G, I = sum(dt_n), sum(gt_n), len(detections)
    dt_f = np.zeros((D, 19), np.float32)                 # box 4, centre 2, z 1, dims 3, pose 9
    gt_f = np.zeros((G, 19), np.float32)                 # box 4, centre 3, dims 3, pose 9
    dt_cat, gt_cat = np.zeros(D, np.int32), np.zeros(G, np.int32)
    K = np.zeros((I, 9), np.float32)
    d = g = 0
    for i, o in enumerate(detections):
        K[i] = np.asarray(o["K"], np.float64).reshape(9)
        for r in o["instances"]:
            dt_f[d, 0:4], dt_f[d, 4:6], dt_f[d, 6] = r["bbox"], r["center_2D"], r["center_cam"][2]
            dt_f[d, 7:10], dt_f[d, 10:19] = r["dimensions"], np.asarray(r["pose"], np.float64).reshape(9)
            dt_cat[d] = r["category_id"]
            d += 1
        for a in dicts[i]["annotations"]:
            mode = a.get("bbox_mode", BoxMode.XYWH_ABS)
            gt_f[g, 0:4] = a["bbox"] if mode == BoxMode.XYWH_ABS else BoxMode.convert(list(a["bbox"]), mode, BoxMode.XYWH_ABS)
            gt_f[g, 4:7], gt_f[g, 7:10], gt_f[g, 10:19] = a["center_cam"], a["dimensions"], np.asarray(a["pose"], np.float64).reshape(9)
            gt_cat[g] = a["category_id"]
            g += 1
    off = lambda n: np.concatenate(([0], np.cumsum(n, dtype=np.int64))).astype(np.int32)      # noqa: E731
    c = np.ascontiguousarray
    return (c(dt_f[:, 0:4]), dt_cat, c(dt_f[:, 4:6]), c(dt_f[:, 6]), c(dt_f[:, 7:10]), c(dt_f[:, 10:19]), off(dt_n),
            c(gt_f[:, 0:4]), gt_cat, c(gt_f[:, 4:7]), c(gt_f[:, 7:10]), c(gt_f[:, 10:19]), off(gt_n), K)


def match_errors_from_instances(detections, dataset):
    """The numbers behind the error line of `visualize_from_instances`: `detections` is the list `inference_on_dataset` returns (and
    `instances_predictions.pth` stores), `dataset` the test loader's dataset in the same order (a sequence of dataset dicts, or an
    object exposing them as `._dataset`).  Every record is packed once on the host, copied once, and matched in one launch of
    csrc/vis_errors.hip (`kernels.viserr.match_errors`, which defines the match and the seven errors).
    -> {"match" (D,) int32 global ground-truth row or -1, "err" (D,7) float32 [xy, z, w, h, l, dim, ry] (NaN where unmatched),
    "dt_off" / "gt_off" (I+1,) int32 (rows of image i), "counts" (matched pairs, pairs with a valid ry), "means" {name: float}} --
    host tensors; a mean over no pair is nan."""
    dicts = _dataset_dicts(dataset)
    packed = [torch.from_numpy(a) for a in _pack_instances(detections, dicts)]
    dev = render.default_device()
    match, err, sums, counts = viserr.match_errors(*[t.to(dev) for t in packed])
    sums, counts = sums.cpu().tolist(), counts.cpu().tolist()
    means = {n: (sums[k] / counts[1 if n == "ry" else 0] if counts[1 if n == "ry" else 0] else float("nan"))
             for k, n in enumerate(viserr.ERR_NAMES)}
    return {"match": match.cpu(), "err": err.cpu(), "dt_off": packed[6], "gt_off": packed[12], "counts": tuple(counts), "means": means}


def _draw_sample(im, K, records, names, thres):
    """the predictions above `thres` onto `im` (numpy HWC uint8, in place): the edges of all boxes in one launch, then the labels"""
    H = im.shape[0]
    thickness = max(1, int(np.round(3 * H / 500)))
    K_inv = np.linalg.inv(K)
    rows, labels = [], []
    for r in records:
        if not r["score"] > thres:
            continue
        z = r["center_cam"][2]
        x3d, y3d, z3d = K_inv @ (z * np.array(list(r["center_2D"]) + [1.0]))
        w3d, h3d, l3d = r["dimensions"]
        color = U.get_color(r["category_id"])
        verts = MU.mesh_cuboid([x3d, y3d, z3d, w3d, h3d, l3d], np.asarray(r["pose"], np.float64)).verts_padded()[0].double().numpy()
        rows += box_segments(K, verts, color, thickness)
        labels.append(("{}, z={:.1f}, s={:.2f}".format(names[r["category_id"]], z3d, r["score"]), r["bbox"], color))
    _draw_rows(im, rows)
    for text, pos, color in labels:
        draw_text(im, text, pos, scale=0.50 * H / 500, bg_color=color)
    return im


def visualize_from_instances(detections, dataset, dataset_name, min_size_test, output_folder, category_names_official, iteration=""):
    """vis.py:76-196, called once per test dataset at the end of every evaluation (tools/train_net.py:99-107).
    1. The log line `<dataset_name>iter=<iteration>, xy(..), z(..), whl(.., .., ..), ry(..)`: the mean errors, in pixels / metres /
       radians, of the predictions matched to a same-category ground-truth box by 2D IoU >= 0.5 (`match_errors_from_instances`).  A
       mean over no pair prints nan, ry without a valid pair prints 1000.00, as in the reference.
    2. Every 50th image that has ground truth is written to `<output_folder>/vis/%06d.jpg` with its predictions scoring above
       sqrt(1 / n_categories): the 3D box (`omni_draw_segments`, colour `util.get_color(category_id)`) and the label
       "<category>, z=.., s=..".  The image is read from `file_name`, or taken from `image_array` where the dataset carries pixels.
    Departures: lines are at least 1 px thick (the reference's int(round(3 H / 500)) is 0 below 84 rows, which cv2.line rejects);
    labels are written after all boxes of the image; the JPEG is written at quality 100 without chroma subsampling (the default
    encoder settings smear a one-pixel line over its 16 x 16 block: up to 110 grey levels two pixels away, 4 with these settings);
    `min_size_test` is accepted and, as in the reference, not used."""
    vis_folder = os.path.join(output_folder, "vis")
    U.mkdir_if_missing(vis_folder)
    dicts = _dataset_dicts(dataset)
    means = match_errors_from_instances(detections, dataset)["means"]
    thres = np.sqrt(1 / len(category_names_official))
    for imind in range(0, len(detections), 50):
        o, entry = detections[imind], dicts[imind]
        if len(entry["annotations"]) == 0:
            continue
        assert entry["image_id"] == o["image_id"]
        im = np.array(entry["image_array"], dtype=np.uint8) if "image_array" in entry else U.imread(entry["file_name"])
        _draw_sample(im, np.asarray(o["K"], np.float64).reshape(3, 3), o["instances"], category_names_official, thres)
        U.imwrite(im, os.path.join(vis_folder, "{:06d}.jpg".format(imind)), quality=100, subsampling=0)
    ry = means["ry"] if means["ry"] == means["ry"] else 1000.0
    return dataset_name + "iter={}, xy({:.2f}), z({:.2f}), whl({:.2f}, {:.2f}, {:.2f}), ry({:.2f})\n".format(
        iteration, means["xy"], means["z"], means["w"], means["h"], means["l"], ry)
