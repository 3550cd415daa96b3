"""Drawing predicted 3D boxes (reference cubercnn/vis/vis.py:210-383, 571-651) on csrc/render.hip: the shaded overlay is a ray cast
against the cuboids (`omni_cuboid_depth` + `omni_scene_compose`) instead of pytorch3d's mesh renderer, the box edges are thick
segments painted by `omni_draw_segments` instead of `cv2.line`.  Images enter and leave as the reference's numpy HWC uint8 arrays;
in between they live on the device as (3,H,W) tensors.  Labels are written last, on the host, with PIL's built-in bitmap font (a
stated departure from OpenCV's Hershey font; not on the hot path)."""
from copy import deepcopy

import numpy as np
import torch

from ...kernels import render
from ..util import math_util as MU

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


def _paint(image, rows):
    if rows:
        render.draw_segments(image, torch.tensor(rows, dtype=torch.float32).to(image.device))


def draw_3d_box_from_verts(im, K, verts3d, color=(0, 200, 200), thickness=1, zplane=0.05, eps=1e-4):
    """vis.py:571-626: the edges of the box with vertices verts3d (8,3, camera space) onto `im`, in place.  im: numpy HWC uint8 (as in
    the reference) or a (3,H,W) uint8 tensor already on the device.  The back / top face highlights are not drawn."""
    rows = box_segments(K, verts3d, color, thickness, zplane, eps)
    if isinstance(im, torch.Tensor):
        _paint(im, rows)
        return im
    dev = _to_device(im)
    _paint(dev, rows)
    im[...] = _to_host(dev)
    return im


def draw_3d_box(im, K, box3d, R, color=(0, 200, 200), thickness=1, view_R=None, view_T=None):
    """vis.py:648-651: box3d [X,Y,Z,W,H,L] with pose R, optionally seen through the rigid motion (view_R, view_T)"""
    verts = MU.mesh_cuboid(box3d, R).verts_padded()[0].double().numpy()
    if view_R is not None:
        verts = (np.asarray(view_R, dtype=np.float64) @ verts.T).T
    if view_T is not None:
        verts = verts + np.asarray(view_T, dtype=np.float64).reshape(1, 3)
    return draw_3d_box_from_verts(im, K, verts, color=color, thickness=thickness)


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


def _shade(image, K, box3d, R, color, blend_weight, zplane):
    dev = image.device
    Kt = torch.tensor(np.asarray(K, dtype=np.float32).reshape(9)).to(dev)
    box3d, R, color = box3d.to(dev), R.to(dev), color.to(dev)
    _, index, face, _, _ = render.cuboid_depth(box3d, R, Kt, image.shape[1], image.shape[2], zplane)
    render.scene_compose(image, index, face, R, Kt, color, blend_weight)
    return index


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
                    blend_weight_overlay=1.0, zplane=0.05):
    """vis.py:210-538.  im: numpy HWC uint8; K: 3x3; meshes: list of `mesh_cuboid` results (one box each, with a colour); text:
    optional label per mesh.  mode '2D_only' -> image with the 2D boxes of the projected vertices; 'front' -> image with the shaded
    boxes blended in by `blend_weight` (skipped at 0), the box edges painted in the reference's order (descending mean y of the vertices), then the whole drawing blended over the
    input by `blend_weight_overlay`; 'novel' -> (view, canvas): the scene rotated about its centre by R (default euler2mat([pi/3, 0, 0]))
    and zoomed with the reference's search (x0.95 per trial, margin 0.01, stop at z < 0.25; `zoom_factor` is used as given when T is
    set) on a white scale x scale canvas; 'front_and_novel' -> (front, view, canvas).  All images are uint8.
    Departures from the reference: the renderer is the ray cast of csrc/render.hip (pixel-centre samples, no specular highlight,
    true depth along the ray); the ground grid of the novel view (vis.py:389-490) is left out; labels are written last, on the host."""
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

    # ---- the novel view (vis.py:315-383, 492-530) ----
    canvas = np.full((scale, scale, 3), 255, dtype=np.uint8)
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
    image = _to_device(canvas)
    _shade(image, K_novel, box_novel, R_novel, colors, 1.0, zplane)
    order = _edges_and_labels(image, K_novel, verts_novel, meshes, max(2, int(np.round(3 * scale / 1250))), zplane)
    im_novel_view = _to_host(image)
    _labels(im_novel_view, K_novel, verts_novel, meshes, text, order)
    if mode == "front_and_novel":
        return im_drawn_rgb, im_novel_view, canvas
    return im_novel_view, canvas
