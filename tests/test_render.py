"""csrc/render.hip (omni_cuboid_depth / omni_scene_compose / omni_draw_segments) and `estimate_visibility` / `render_depth_map`
against float64 references written here from the definitions, by a method the kernels do not use: the cast kernel clips the pixel
ray against the three slabs of a box in the box frame; the reference builds the 12 triangles of `get_cuboid_verts_faces` and
intersects every pixel ray with every triangle (Moeller-Trumbore), keeping the nearest hit at depth >= zplane.  pytorch3d and
OpenCV are not installed, so pixel parity with the reference's renderer cannot be pinned (same position as oracle/upstream.py).

`index` and `face` must equal the reference exactly; `depth` is held to max(3 x the distance of the SAME reference evaluated in
float32 from the float64 one, one fp32 ulp of the largest depth), distances measured as |a - b| / (1 + |b|).  A pixel is left out of
the comparison only when, in the float64 reference, its sample point lies within 1e-3 px of a projected edge of a triangle of any
box (of the part of the triangle at depth >= zplane, which is all the reference keeps of it), or when its two nearest hits differ by
less than 1e-5 relative (the hand-placed pair with the identical front face excepted: there the lower index must win).  The
left-out pixels are at most 0.5 % of the covered pixels of every case (asserted; met by the chosen seeds with the reference alone).
Per box, `area` and `visible` may differ from the reference by at most the left-out pixels inside the box's rectangle.

Measured distances of depth to float64, largest over the cases (kernel | float32 reference), under the host emulator:
8.3e-07 | 6.4e-07 (the 50 x 70, 70-box case; 1.3e-07 .. 4.7e-07 | 2.4e-07 .. 5.2e-07 in the others).
"""
import functools

import numpy as np
import pytest
import torch

ZPLANE = 0.05
FACES = np.array([[0, 1, 2], [2, 3, 0], [1, 5, 6], [6, 2, 1], [4, 0, 3], [3, 7, 4], [5, 4, 7], [7, 6, 5], [4, 5, 1], [1, 0, 4],
                  [3, 2, 6], [6, 7, 3]])
EDGE_TOL, TIE_TOL, LEFT_OUT_CAP = 1e-3, 1e-5, 0.005
VIEWS = ((96, 128), (50, 70))         # (H, W); the second leaves partial tiles on both edges
COUNTS = (1, 7, 70)                   # random boxes; 70 + the hand-placed ones is more than one LDS chunk of 64
SEEDS = {(96, 128, 1): 11, (96, 128, 7): 12, (96, 128, 70): 30, (50, 70, 1): 21, (50, 70, 7): 22, (50, 70, 70): 30, (50, 70, -7): 24}


def _intrinsics(H, W):
    return np.array([[0.9 * W + 0.3, 0.0, 0.5 * W + 1.7], [0.0, 0.9 * W - 0.4, 0.5 * H - 0.9], [0.0, 0.0, 1.0]])


def _rot(a, b, c):
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _scene(H, W, n):
    """n random boxes (n < 0: -n random boxes only) + the hand-placed ones -> box3d (N,6) float32, R (N,3,3) float32, names -> row"""
    rs = np.random.RandomState(SEEDS[(H, W, n)])
    K = _intrinsics(H, W)
    boxes, rots = [], []
    for _ in range(abs(n)):
        z = rs.uniform(1.0, 8.0)
        # projected centres spread over three view widths / heights: most boxes are culled, some cross the border
        u, v = rs.uniform(-1.0 * W, 2.0 * W), rs.uniform(-1.0 * H, 2.0 * H)
        if abs(n) == 1:
            u, v = rs.uniform(0.3 * W, 0.7 * W), rs.uniform(0.3 * H, 0.7 * H)
        boxes.append([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z] + list(rs.uniform(0.2, 2.0, size=3)))
        rots.append(_rot(rs.uniform(-np.pi, np.pi), rs.uniform(-0.6, 0.6), rs.uniform(-0.6, 0.6)))
    names = {}
    if n > 0:
        eye = np.eye(3)
        hand = [("straddle", [-0.30, -0.20, 0.30, 0.70, 0.25, 0.35], _rot(0.3, 0.2, -0.1)),  # z from about -0.1 to 0.7: crosses zplane
                ("inside", [0.2, -0.1, 0.5, 21.0, 9.0, 13.0], _rot(0.5, -0.3, 0.2)),       # the camera is inside
                ("behind", [0.1, 0.2, -3.0, 1.0, 1.0, 1.0], _rot(1.0, 0.1, 0.3)),          # wholly behind the camera
                ("outside", [40.0, 1.0, 5.0, 1.0, 1.0, 1.0], _rot(-0.7, 0.2, 0.1)),        # wholly outside the frustum
                ("tie_a", [0.125, -0.0625, 4.0, 1.0, 0.75, 1.5], eye),                     # front face z = 3.5 ...
                ("tie_b", [0.125, -0.0625, 4.5, 2.0, 0.75, 1.5], eye)]                     # ... and the same front face again
        for name, b, r in hand:
            names[name] = len(boxes)
            boxes.append(b)
            rots.append(r)
    return np.asarray(boxes, np.float32), np.asarray(rots, np.float32), K.astype(np.float32), names


def _verts(box3d, R):
    """get_cuboid_verts_faces (math_util.py:116-219) in the dtype of its arguments -> (N,8,3)"""
    dt = box3d.dtype
    sx = np.array([-1, 1, 1, -1, -1, 1, 1, -1], dt) * 0.5
    sy = np.array([-1, -1, 1, 1, -1, -1, 1, 1], dt) * 0.5
    sz = np.array([-1, -1, -1, -1, 1, 1, 1, 1], dt) * 0.5
    local = np.stack((box3d[:, 5:6] * sx, box3d[:, 4:5] * sy, box3d[:, 3:4] * sz), axis=1)      # (N,3,8)
    return (np.matmul(R, local) + box3d[:, :3, None]).transpose(0, 2, 1)


def _rays(K, ys, xs):
    dt = K.dtype
    dy = (ys.astype(dt) + dt.type(0.5) - K[1, 2]) / K[1, 1]
    dx = (xs.astype(dt) + dt.type(0.5) - K[0, 2] - K[0, 1] * dy) / K[0, 0]
    return np.stack((dx, dy, np.ones_like(dx)), axis=-1)


def _rect(verts, K, H, W):
    """inclusive pixel rectangle (x0, y0, x1, y1) that holds every pixel a box can cover; None: the box covers nothing"""
    z = verts[:, 2]
    if z.max() < ZPLANE:
        return None
    if z.min() < ZPLANE:
        return 0, 0, W - 1, H - 1
    u = (K[0, 0] * verts[:, 0] + K[0, 1] * verts[:, 1]) / z + K[0, 2]
    v = K[1, 1] * verts[:, 1] / z + K[1, 2]
    x0, x1 = max(int(np.floor(u.min())) - 2, 0), min(int(np.ceil(u.max())) + 2, W - 1)
    y0, y1 = max(int(np.floor(v.min())) - 2, 0), min(int(np.ceil(v.max())) + 2, H - 1)
    return (x0, y0, x1, y1) if x0 <= x1 and y0 <= y1 else None


def _cast_reference(box3d, R, K, H, W, dt, rects):
    """Moeller-Trumbore over the 12 triangles of every box, all arithmetic in `dt` -> per-box depth (N,H,W) (+inf: no hit at depth >=
    zplane) and face (N,H,W)"""
    box3d, R, K = box3d.astype(dt), R.astype(dt), K.astype(dt)
    verts = _verts(box3d, R)
    N = len(box3d)
    depth = np.full((N, H, W), np.inf, dt)
    face = np.full((N, H, W), -1, np.int32)
    zp = dt(ZPLANE)
    for b in range(N):
        if rects[b] is None:
            continue
        x0, y0, x1, y1 = rects[b]
        ys, xs = np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), indexing="ij")
        d = _rays(K, ys, xs)[:, :, None, :]                                  # (h,w,1,3)
        tri = verts[b][FACES]                                                # (12,3,3)
        v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        p = np.cross(d, e2)                                                  # (h,w,12,3)
        det = (e1 * p).sum(-1)
        ok = det != 0
        inv = 1.0 / np.where(ok, det, dt(1))
        tvec = -v0                                                           # the ray starts at the camera centre
        u = (tvec * p).sum(-1) * inv
        q = np.cross(tvec, e1)                                               # (12,3)
        v = (d * q).sum(-1) * inv
        t = (e2 * q).sum(-1) * inv
        hit = ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= zp)
        t = np.where(hit, t, dt(np.inf))
        k = t.argmin(-1)
        tb = np.take_along_axis(t, k[..., None], -1)[..., 0]
        depth[b, y0:y1 + 1, x0:x1 + 1] = tb
        face[b, y0:y1 + 1, x0:x1 + 1] = np.where(np.isfinite(tb), k // 2, -1)
    return depth, face


def _near_edges(box3d, R, K, H, W, rects):
    """(H,W) bool: the sample point lies within EDGE_TOL px of a projected edge of a triangle, clipped to depth >= zplane"""
    verts = _verts(box3d.astype(np.float64), R.astype(np.float64))
    K = K.astype(np.float64)
    near = np.zeros((H, W), bool)
    for b in range(len(box3d)):
        if rects[b] is None:
            continue
        for tri in verts[b][FACES]:
            poly = []
            for i in range(3):                                               # Sutherland-Hodgman against z >= zplane
                a, c = tri[i], tri[(i + 1) % 3]
                if a[2] >= ZPLANE:
                    poly.append(a)
                if (a[2] >= ZPLANE) != (c[2] >= ZPLANE):
                    poly.append(a + (ZPLANE - a[2]) / (c[2] - a[2]) * (c - a))
            if len(poly) < 2:
                continue
            pts = np.array([[(K[0, 0] * p[0] + K[0, 1] * p[1]) / p[2] + K[0, 2], K[1, 1] * p[1] / p[2] + K[1, 2]] for p in poly])
            for i in range(len(pts)):
                a, c = pts[i], pts[(i + 1) % len(pts)]
                x0, x1 = int(np.floor(min(a[0], c[0]) - 1.5)), int(np.ceil(max(a[0], c[0]) + 0.5))
                y0, y1 = int(np.floor(min(a[1], c[1]) - 1.5)), int(np.ceil(max(a[1], c[1]) + 0.5))
                x0, x1, y0, y1 = max(x0, 0), min(x1, W - 1), max(y0, 0), min(y1, H - 1)
                if x0 > x1 or y0 > y1:
                    continue
                ys, xs = np.meshgrid(np.arange(y0, y1 + 1) + 0.5, np.arange(x0, x1 + 1) + 0.5, indexing="ij")
                e = c - a
                l2 = float(e @ e)
                s = np.clip(((xs - a[0]) * e[0] + (ys - a[1]) * e[1]) / l2, 0.0, 1.0) if l2 > 0 else np.zeros_like(xs)
                dist = np.hypot(xs - a[0] - s * e[0], ys - a[1] - s * e[1])
                near[y0:y1 + 1, x0:x1 + 1] |= dist <= EDGE_TOL
    return near


@functools.lru_cache(maxsize=None)
def _case(H, W, n):
    """the scene and its float64 / float32 references, computed once and shared (never written to)"""
    box3d, R, K, names = _scene(H, W, n)
    N = len(box3d)
    verts = _verts(box3d.astype(np.float64), R.astype(np.float64))
    rects = [_rect(verts[b], K.astype(np.float64), H, W) for b in range(N)]
    d64, f64 = _cast_reference(box3d, R, K, H, W, np.float64, rects)
    d32, _ = _cast_reference(box3d, R, K, H, W, np.float32, rects)
    index = d64.argmin(0).astype(np.int32)                    # the first minimum: equal depths go to the lower index
    depth = np.take_along_axis(d64, index[None].astype(np.int64), 0)[0]
    covered = np.isfinite(depth)
    index[~covered] = -1
    face = np.where(covered, np.take_along_axis(f64, np.maximum(index, 0)[None].astype(np.int64), 0)[0], -1).astype(np.int32)
    depth32 = np.take_along_axis(d32, np.maximum(index, 0)[None].astype(np.int64), 0)[0]      # the SAME hit, evaluated in float32
    # left-out pixels
    out = _near_edges(box3d, R, K, H, W, rects)
    if N > 1:
        two = np.sort(d64, axis=0)[:2]
        order = np.argsort(d64, axis=0, kind="stable")[:2]
        with np.errstate(invalid="ignore"):
            close = np.isfinite(two[1]) & ((two[1] - two[0]) < TIE_TOL * two[0])
        if "tie_a" in names:
            pair = (np.minimum(order[0], order[1]) == names["tie_a"]) & (np.maximum(order[0], order[1]) == names["tie_b"])
            close &= ~pair
        out |= close
    hit = np.isfinite(d64)
    area = hit.sum((1, 2)).astype(np.int64)
    visible = np.array([(index == b).sum() for b in range(N)], np.int64)
    slack = np.array([0 if r is None else int(out[r[1]:r[3] + 1, r[0]:r[2] + 1].sum()) for r in rects], np.int64)
    for a in (depth, index, face, depth32, out, area, visible, slack):
        a.setflags(write=False)
    return dict(box3d=box3d, R=R, K=K, names=names, depth=depth, index=index, face=face, depth32=depth32, out=out, covered=covered,
                area=area, visible=visible, slack=slack, H=H, W=W)


CASES = [(H, W, n) for (H, W) in VIEWS for n in COUNTS] + [(50, 70, -7)]        # the last: no hand-placed box, so background shows


@pytest.mark.parametrize("H,W,n", CASES)
def test_left_out_pixels_stay_under_the_cap(H, W, n):
    """a condition on the chosen seeds, checked with the reference alone"""
    c = _case(H, W, n)
    assert c["covered"].sum() > 0
    assert c["out"].sum() <= LEFT_OUT_CAP * c["covered"].sum(), (int(c["out"].sum()), int(c["covered"].sum()))
    if n > 0:
        nm = c["names"]
        assert c["covered"].all()                                             # the box around the camera is seen everywhere
        assert c["area"][nm["behind"]] == 0 and c["area"][nm["outside"]] == 0
        assert c["visible"][nm["tie_a"]] > 0 and c["visible"][nm["tie_b"]] == 0 and c["area"][nm["tie_b"]] >= c["area"][nm["tie_a"]] > 0
        assert (c["face"][c["index"] == nm["inside"]] >= 0).all()
    else:
        assert not c["covered"].all()


def _dist(a, b):
    return float((np.abs(a - b) / (1.0 + np.abs(b))).max())


def _run_cast(dev, H, W, n):
    from omni3d_amd.kernels import render
    c = _case(H, W, n)
    t = lambda a: torch.tensor(a).to(dev)            # noqa: E731
    outs = [render.cuboid_depth(t(c["box3d"]), t(c["R"]), t(c["K"]), H, W, ZPLANE) for _ in range(2)]
    for a, b in zip(*outs):
        assert torch.equal(a, b)                                             # two runs are bit-identical
    depth, index, face, area, visible = [o.cpu().numpy() for o in outs[0]]
    keep = ~c["out"]
    assert c["out"].sum() <= LEFT_OUT_CAP * c["covered"].sum()
    assert np.array_equal(index[keep], c["index"][keep]), int((index != c["index"])[keep].sum())
    assert np.array_equal(face[keep], c["face"][keep]), int((face != c["face"])[keep].sum())
    bg = keep & ~c["covered"]
    assert np.all(np.isposinf(depth[bg]))
    m = keep & c["covered"]
    e_hip, e_ref = _dist(depth[m].astype(np.float64), c["depth"][m]), _dist(c["depth32"][m].astype(np.float64), c["depth"][m])
    ulp = float(np.spacing(np.float32(c["depth"][m].max()))) / (1.0 + float(c["depth"][m].max()))
    print("cast %dx%d n=%d: |hip-fp64| %.2e  |ref32-fp64| %.2e  left out %d of %d covered" % (H, W, n, e_hip, e_ref, c["out"].sum(), c["covered"].sum()))
    assert e_hip <= max(3.0 * e_ref, ulp), (e_hip, e_ref, ulp)
    for name, got in (("area", area), ("visible", visible)):
        diff = np.abs(got.astype(np.int64) - c[name])
        assert (diff <= c["slack"]).all(), (name, got.tolist(), c[name].tolist(), c["slack"].tolist())
    return e_hip, e_ref


@pytest.mark.parametrize("H,W,n", CASES)
def test_cuboid_depth_emulated(emu_lib, H, W, n):
    _run_cast("cpu", H, W, n)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,n", CASES)
def test_cuboid_depth_gpu(hip_lib, H, W, n):
    _run_cast("cuda", H, W, n)


# ---- estimate_visibility / render_depth_map ------------------------------------------------------------------------------------

def _run_visibility(dev):
    from omni3d_amd.cubercnn.util import math_util as MU
    H, W, n = 50, 70, 7
    c = _case(H, W, n)
    K = c["K"].reshape(3, 3)
    vis = MU.estimate_visibility(K, torch.from_numpy(c["box3d"]), torch.from_numpy(c["R"]), W, H, device=dev)
    assert len(vis) == len(c["box3d"])
    for b, v in enumerate(vis):
        a, s, slack = int(c["area"][b]), int(c["visible"][b]), int(c["slack"][b])
        if a == 0 and slack == 0:
            assert np.isnan(v), (b, v)
        elif slack == 0:
            assert v == np.float32(s) / np.float32(a), (b, v, s, a)
        elif a > slack:
            assert (s - slack) / (a + slack) <= v <= (s + slack) / (a - slack), (b, v, s, a, slack)
    assert np.isnan(vis[c["names"]["behind"]])
    sil, depth_map, inds = MU.render_depth_map(K, torch.from_numpy(c["box3d"]), torch.from_numpy(c["R"]), W, H, device=dev)
    assert sil.shape == (len(c["box3d"]), H, W) and sil.dtype == torch.bool and depth_map.shape == (H, W) and inds.shape == (H, W)
    keep = ~c["out"]
    assert np.array_equal(inds.cpu().numpy()[keep], c["index"][keep])
    for b in range(len(c["box3d"])):
        assert abs(int(sil[b].sum()) - int(c["area"][b])) <= int(c["slack"][b])
    # a lone box is wholly visible; a box half behind a nearer one is partly visible
    eye = torch.eye(3).reshape(1, 3, 3)
    Kf = np.array([[60.0, 0, 35.0], [0, 60.0, 25.0], [0, 0, 1]])
    one = MU.estimate_visibility(Kf, torch.tensor([[0.0, 0.0, 4.0, 1.0, 1.0, 1.0]]), eye, 70, 50, device=dev)
    assert one == [1.0]
    two = MU.estimate_visibility(Kf, torch.tensor([[0.0, 0.0, 4.0, 1.0, 1.0, 1.0], [0.5, 0.0, 2.5, 0.5, 1.5, 1.0]]), eye.repeat(2, 1, 1), 70, 50,
                                 device=dev)
    assert 0.0 < two[0] < 1.0 and two[1] == 1.0, two


def test_estimate_visibility_emulated(emu_lib):
    _run_visibility("cpu")


@pytest.mark.gpu
def test_estimate_visibility_gpu(hip_lib):
    _run_visibility("cuda")


# ---- omni_scene_compose --------------------------------------------------------------------------------------------------------

def _shade_reference(c, color, image, blend):
    """out = shaded * blend + image * (1 - blend), shaded = 255 * colour * (0.5 + 0.3 * max(0, n . l)), float64, not rounded"""
    H, W = c["H"], c["W"]
    K, R = c["K"].astype(np.float64), c["R"].astype(np.float64)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = _rays(K, ys, xs)
    idx = np.maximum(c["index"], 0)
    axis = np.array([2, 0, 0, 2, 1, 1])[np.maximum(c["face"], 0)]            # front/back: width axis, right/left: length, top/bottom: height
    sign = np.array([-1.0, 1.0, -1.0, 1.0, -1.0, 1.0])[np.maximum(c["face"], 0)]
    nrm = sign[..., None] * R[idx, :, axis]                                  # outward normal = +- a column of R
    p = d * c["depth"][..., None].clip(max=1e30)                             # hit point; the light sits at the camera centre
    inward = (nrm * d).sum(-1) > 0
    nrm = np.where(inward[..., None], -nrm, nrm)                             # exit face: seen from inside
    with np.errstate(invalid="ignore"):
        l = -p / np.linalg.norm(p, axis=-1, keepdims=True)
    shade = 0.5 + 0.3 * np.maximum((nrm * l).sum(-1), 0.0)
    shaded = 255.0 * color.astype(np.float64)[idx].transpose(2, 0, 1) * shade[None]
    out = shaded * blend + image.astype(np.float64) * (1.0 - blend)
    return np.where(c["covered"][None], out, image.astype(np.float64))


def _run_compose(dev):
    from omni3d_amd.kernels import render
    for (H, W, n) in ((96, 128, 7), (50, 70, -7)):
        c = _case(H, W, n)
        rs = np.random.RandomState(5)
        image = rs.randint(0, 256, size=(3, H, W)).astype(np.uint8)
        color = rs.uniform(0.1, 1.0, size=(len(c["box3d"]), 3)).astype(np.float32)
        t = lambda a: torch.tensor(a).to(dev)        # noqa: E731
        for blend in (0.0, 0.5, 0.8, 1.0):
            got = render.scene_compose(t(image), t(c["index"]), t(c["face"]), t(c["R"]), t(c["K"]), t(color), blend).cpu().numpy()
            want = _shade_reference(c, color, image, blend)
            keep = np.broadcast_to(~c["out"], got.shape)
            assert np.abs(got.astype(np.float64) - want)[keep].max() <= 1.0
            assert np.array_equal(got[:, ~c["covered"]], image[:, ~c["covered"]])
            if blend == 0.0:
                assert np.array_equal(got, image)
            if blend == 1.0:
                shaded = _shade_reference(c, color, np.zeros_like(image), 1.0)
                m = np.broadcast_to(c["covered"] & ~c["out"], got.shape)
                assert np.abs(got.astype(np.float64) - shaded)[m].max() <= 1.0


def test_scene_compose_emulated(emu_lib):
    _run_compose("cpu")


@pytest.mark.gpu
def test_scene_compose_gpu(hip_lib):
    _run_compose("cuda")


# ---- omni_draw_segments --------------------------------------------------------------------------------------------------------

SEG_H, SEG_W = 64, 80


def _segment_sets():
    base = [
        (5.2, 10.3, 70.4, 10.3, 1.0, 255, 0, 0),            # horizontal
        (12.7, 3.1, 12.7, 60.2, 2.0, 0, 255, 0),            # vertical
        (3.2, 4.1, 60.7, 50.3, 5.0, 0, 0, 255),             # diagonal
        (70.3, 5.2, 20.9, 61.4, 2.0, 200, 200, 0),          # the other diagonal
        (40.3, 30.8, 40.3, 30.8, 5.0, 9, 99, 199),          # zero length: a disc
        (60.4, 40.2, 120.0, 75.0, 2.0, 50, 60, 70),         # leaves the image
        (-40.0, -9.0, -3.0, -30.0, 5.0, 1, 2, 3),           # wholly outside
        (10.3, 55.6, 75.2, 20.1, 1.0, 250, 128, 3),         # crosses several of the above
    ]
    cross_a, cross_b = (20.2, 20.4, 60.1, 44.9, 5.0, 10, 20, 30), (20.6, 45.2, 61.3, 19.7, 5.0, 40, 50, 60)
    rs = np.random.RandomState(3)
    many = []
    for _ in range(150 - len(base) - 2):                    # short strokes all over the image and a little beyond it
        x0, y0 = rs.uniform(-8, SEG_W + 8), rs.uniform(-8, SEG_H + 8)
        many.append((x0, y0, x0 + rs.uniform(-12, 12), y0 + rs.uniform(-12, 12), float(rs.choice([1.0, 2.0, 5.0]))) +
                    tuple(float(v) for v in rs.randint(0, 256, 3)))
    return {"one": [base[2]], "cross_ab": base + [cross_a, cross_b], "cross_ba": base + [cross_b, cross_a],
            "150": base[:4] + many + base[4:] + [cross_a, cross_b]}


def _segments_reference(segs, image):
    """float64 capsule test -> (painted image, pixels whose centre is within EDGE_TOL px of a capsule boundary)"""
    out = image.copy()
    ys, xs = np.meshgrid(np.arange(SEG_H) + 0.5, np.arange(SEG_W) + 0.5, indexing="ij")
    unsure = np.zeros((SEG_H, SEG_W), bool)
    for x0, y0, x1, y1, th, r, g, b in np.asarray(segs, np.float32).astype(np.float64):
        ex, ey = x1 - x0, y1 - y0
        l2 = ex * ex + ey * ey
        s = np.clip(((xs - x0) * ex + (ys - y0) * ey) / l2, 0.0, 1.0) if l2 > 0 else np.zeros_like(xs)
        dist = np.hypot(xs - x0 - s * ex, ys - y0 - s * ey)
        inside = dist <= th / 2
        unsure |= np.abs(dist - th / 2) <= EDGE_TOL
        for ch, v in enumerate((r, g, b)):
            out[ch][inside] = v
    return out, unsure


def _run_segments(dev):
    from omni3d_amd.kernels import render
    rs = np.random.RandomState(9)
    image = rs.randint(0, 256, size=(3, SEG_H, SEG_W)).astype(np.uint8)
    sets = _segment_sets()
    assert len(sets["one"]) == 1 and len(sets["150"]) == 150
    painted = {}
    for name, segs in sets.items():
        want, unsure = _segments_reference(segs, image)
        drawn = (want != image).any(0)
        assert unsure.sum() <= LEFT_OUT_CAP * max(int(drawn.sum()), 1), (name, int(unsure.sum()), int(drawn.sum()))
        got = render.draw_segments(torch.from_numpy(image.copy()).to(dev), torch.tensor(segs, dtype=torch.float32).to(dev)).cpu().numpy()
        assert np.array_equal(got[:, ~unsure], want[:, ~unsure]), (name, int((got != want).any(0)[~unsure].sum()))
        painted[name] = got
    # the later of two crossing segments wins, in both list orders
    assert tuple(painted["cross_ab"][:, 32, 40]) == (40, 50, 60) and tuple(painted["cross_ba"][:, 32, 40]) == (10, 20, 30)


def test_draw_segments_emulated(emu_lib):
    _run_segments("cpu")


@pytest.mark.gpu
def test_draw_segments_gpu(hip_lib):
    _run_segments("cuda")
