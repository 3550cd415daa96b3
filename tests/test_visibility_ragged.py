"""csrc/annotate.hip `omni_visibility_ragged` (`kernels.annotate.visibility_ragged`): the `area` / `visible` counters of every box
of every image of a ragged scene in one launch,
(a) against `render.cuboid_depth` called once per image on the same library: equal box by box.  Under the host emulator with no
    exception (the same source on the same host arithmetic).  On the GPU a differing count is accepted only on a box where (b)
    lists ambiguous pixels, and by no more than their number: the compiler may contract the shared functions differently in the two
    kernels.  No MI355X run has been taken yet, so whether any count differs there is not known.
(b) against a float64 slab cast written here in numpy (vectorised over the pixels of an image).  A pixel is ambiguous for a box when,
    in float64, |tn - tf| < 1e-4 (1 + |tf|), or |tf - zplane| < 1e-4, or |tn - zplane| < 1e-4 for that box, or when the two nearest
    hit depths of the pixel differ by less than 1e-5 relative and the box is one of the two (identical boxes excepted: there the
    lower row must win).  Per box, |area - ref| and |visible - ref| may not exceed its ambiguous pixels, and the ambiguous pixels
    are at most 0.5 % of the covered pixels of a case (met by the chosen seeds with the reference alone, asserted).
(c) two launches give the same bits; an image without boxes, I == 0 and N == 0 work; an image alone gives the rows it has in the
    whole scene; permuted images give permuted counters.
"""
import functools

import numpy as np
import pytest
import torch

ZPLANE = 0.05
SIZES = ((33, 17), (50, 40), (16, 16), (30, 20), (47, 31), (640, 480), (21, 37))        # (W, H)
COUNTS = (5, 65, 1, 0, 130, 5, 65)                                                        # 65, 130: more than one LDS chunk of 64, partial last chunk
HAND_IMAGE, INSIDE_IMAGE = 4, 0
SEEDS = (2, 9)
GRAZE_TOL, PLANE_TOL, TIE_TOL, AMBIGUOUS_CAP = 1e-4, 1e-4, 1e-5, 0.005
ARGS = ("box3d", "R", "box_off", "K", "size")


def _intrinsics(W, H):
    return np.array([[0.9 * W + 0.3, 0.0, 0.5 * W + 1.7], [0.0, 0.9 * W - 0.4, 0.5 * H - 0.9], [0.0, 0.0, 1.0]])


def _rot(a, b, c):
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _scene(seed):
    rs = np.random.RandomState(seed)
    boxes, rots, Ks, names = [], [], [], {}
    for i, ((W, H), n) in enumerate(zip(SIZES, COUNTS)):
        K = _intrinsics(W, H)
        Ks.append(K)
        first = len(boxes)
        for _ in range(n):
            z = rs.uniform(1.0, 8.0)
            u, v = (rs.uniform(-0.5 * W, 1.5 * W), rs.uniform(-0.5 * H, 1.5 * H)) if n > 1 else (rs.uniform(0.3 * W, 0.7 * W), rs.uniform(0.3 * H, 0.7 * H))
            boxes.append([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z] + list(rs.uniform(0.2, 2.0, size=3)))
            rots.append(_rot(rs.uniform(-np.pi, np.pi), rs.uniform(-0.6, 0.6), rs.uniform(-0.6, 0.6)))
        if i == HAND_IMAGE:                   # hand-placed rows replace random ones; 62 .. 65 straddle the first LDS chunk
            eye = np.eye(3)
            hand = [(3, "straddle", [-0.30, -0.20, 0.30, 0.70, 0.25, 0.35], _rot(0.3, 0.2, -0.1)),   # z from about -0.1 to 0.7: crosses zplane
                    (7, "behind", [0.1, 0.2, -3.0, 1.0, 1.0, 1.0], _rot(1.0, 0.1, 0.3)),           # wholly behind the camera
                    (63, "tie_a", [0.125, -0.0625, 0.4375, 0.125, 0.125, 0.125], eye),                     # two identical boxes, one in each chunk
                    (64, "tie_b", [0.125, -0.0625, 0.4375, 0.125, 0.125, 0.125], eye)]
            for k, name, b, r in hand:
                boxes[first + k], rots[first + k], names[name] = b, r, first + k
        if i == INSIDE_IMAGE:                 # the camera is inside the last box of this image: seen wherever nothing stands in front
            boxes[-1], rots[-1], names["inside"] = [0.2, -0.1, 0.5, 21.0, 9.0, 13.0], _rot(0.5, -0.3, 0.2), len(boxes) - 1
    return dict(box3d=np.asarray(boxes, np.float32).reshape(-1, 6), R=np.asarray(rots, np.float32).reshape(-1, 9),
                box_off=np.concatenate(([0], np.cumsum(COUNTS))).astype(np.int32), K=np.asarray(Ks, np.float32).reshape(-1, 9),
                size=np.asarray(SIZES, np.int32)), names


def _cast64(box3d, R, K, W, H):
    """float64 slab cast of the float32 inputs of one image -> depth (N,H,W) (+inf: no hit), own (N,H,W) bool: the pixel is
    ambiguous for the box by its own entry / exit depths"""
    box3d, R, K = box3d.astype(np.float64), R.astype(np.float64).reshape(-1, 3, 3), K.astype(np.float64).reshape(3, 3)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    dy = (ys + 0.5 - K[1, 2]) / K[1, 1]
    dx = (xs + 0.5 - K[0, 2] - K[0, 1] * dy) / K[0, 0]
    d = np.stack((dx, dy, np.ones_like(dx)), axis=-1)                                      # (H,W,3)
    N = len(box3d)
    depth, own = np.full((N, H, W), np.inf), np.zeros((N, H, W), bool)
    for b in range(N):
        half = 0.5 * box3d[b, [5, 4, 3]]
        o = -(R[b].T @ box3d[b, :3])                                                       # the camera centre in the box frame
        l = d @ R[b]                                                                       # (H,W,3): R^T d
        tn, tf, ok = np.full((H, W), -np.inf), np.full((H, W), np.inf), np.ones((H, W), bool)
        for a in range(3):
            par = l[..., a] == 0
            inv = 1.0 / np.where(par, 1.0, l[..., a])
            ta, tb = (-half[a] - o[a]) * inv, (half[a] - o[a]) * inv
            tn = np.where(par, tn, np.maximum(tn, np.minimum(ta, tb)))
            tf = np.where(par, tf, np.minimum(tf, np.maximum(ta, tb)))
            ok &= ~par | (abs(o[a]) <= half[a])
        hit = ok & (tn <= tf) & (tf >= ZPLANE)
        depth[b] = np.where(hit, np.where(tn >= ZPLANE, tn, tf), np.inf)
        with np.errstate(invalid="ignore"):
            own[b] = ok & ((np.abs(tn - tf) < GRAZE_TOL * (1 + np.abs(tf))) | (np.abs(tf - ZPLANE) < PLANE_TOL) | (np.abs(tn - ZPLANE) < PLANE_TOL))
    return depth, own


@functools.lru_cache(maxsize=None)
def _case(seed):
    """the scene and its float64 counters, computed once and shared (never written to)"""
    a, names = _scene(seed)
    N = len(a["box3d"])
    area, visible, amb, covered, amb_px = np.zeros(N, np.int64), np.zeros(N, np.int64), np.zeros(N, np.int64), 0, 0
    for i, (W, H) in enumerate(SIZES):
        b0, b1 = int(a["box_off"][i]), int(a["box_off"][i + 1])
        if b0 == b1:
            continue
        depth, own = _cast64(a["box3d"][b0:b1], a["R"][b0:b1], a["K"][i], W, H)
        hit = np.isfinite(depth)
        win = depth.argmin(0)                                                              # the first minimum: equal depths go to the lower row
        any_hit = hit.any(0)
        area[b0:b1] = hit.sum((1, 2))
        visible[b0:b1] = np.bincount(win[any_hit], minlength=b1 - b0)
        ambiguous = own.copy()
        if b1 - b0 > 1:
            order = np.argsort(depth, axis=0, kind="stable")[:2]
            two = np.take_along_axis(depth, order, 0)
            with np.errstate(invalid="ignore"):
                close = np.isfinite(two[1]) & ((two[1] - two[0]) < TIE_TOL * np.abs(two[0]))
            same = (a["box3d"][b0:b1][order[0]] == a["box3d"][b0:b1][order[1]]).all(-1) & (a["R"][b0:b1][order[0]] == a["R"][b0:b1][order[1]]).all(-1)
            close &= ~same
            for k in range(2):
                ys, xs = np.nonzero(close)
                ambiguous[order[k][ys, xs], ys, xs] = True
        amb[b0:b1] = ambiguous.sum((1, 2))
        covered += int(any_hit.sum())
        amb_px += int(ambiguous.any(0).sum())
    out = dict(a, area=area, visible=visible, ambiguous=amb, covered=np.int64(covered), ambiguous_pixels=np.int64(amb_px),
               **{"row_" + k: np.int64(v) for k, v in names.items()})
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@pytest.mark.parametrize("seed", SEEDS)
def test_reference_alone_meets_the_conditions(seed):
    """conditions on the chosen seeds and on the hand-placed rows, checked with the float64 reference alone"""
    c = _case(seed)
    assert len(SIZES) <= 10 and set(COUNTS) == {0, 1, 5, 65, 130}
    assert c["ambiguous_pixels"] <= AMBIGUOUS_CAP * c["covered"], (int(c["ambiguous_pixels"]), int(c["covered"]))
    area, vis = c["area"], c["visible"]
    W, H = SIZES[INSIDE_IMAGE]
    assert area[c["row_behind"]] == 0 and vis[c["row_behind"]] == 0
    assert area[c["row_inside"]] == W * H and 0 < vis[c["row_inside"]] < W * H            # seen from inside wherever nothing is in front
    assert area[c["row_straddle"]] > 0
    assert area[c["row_tie_a"]] == area[c["row_tie_b"]] > 0 and vis[c["row_tie_a"]] > 0 and vis[c["row_tie_b"]] == 0
    assert (vis <= area).all() and (area > 0).sum() > 60 and ((vis < area) & (vis > 0)).sum() > 10
    off = c["box_off"]
    for i in range(len(SIZES)):                                                            # every image with boxes shows some
        assert off[i] == off[i + 1] or area[off[i]:off[i + 1]].sum() > 0


def _t(c, dev, keys=ARGS):
    return [torch.from_numpy(np.array(c[k])).to(dev) for k in keys]


def _per_image(dev, c):
    """the counters of render.cuboid_depth, one call per image"""
    from omni3d_amd.kernels import render
    area, visible = np.zeros(len(c["box3d"]), np.int32), np.zeros(len(c["box3d"]), np.int32)
    box3d, R, K = _t(c, dev, ("box3d", "R", "K"))
    for i, (W, H) in enumerate(np.array(c["size"]).tolist()):
        b0, b1 = int(c["box_off"][i]), int(c["box_off"][i + 1])
        if b1 > b0:
            out = render.cuboid_depth(box3d[b0:b1], R[b0:b1], K[i], H, W, ZPLANE)
            area[b0:b1], visible[b0:b1] = out[3].cpu().numpy(), out[4].cpu().numpy()
    return area, visible


def _run_case(dev, seed, exact):
    from omni3d_amd.kernels import annotate
    c = _case(seed)
    outs = [annotate.visibility_ragged(*_t(c, dev), zplane=ZPLANE) for _ in range(2)]
    for x, y in zip(*outs):
        assert x.dtype == torch.int32 and torch.equal(x.cpu(), y.cpu())                    # two launches are bit-identical
    area, visible = [o.cpu().numpy() for o in outs[0]]
    # (b) the float64 cast
    da, dv = np.abs(area - c["area"]), np.abs(visible - c["visible"])
    print("seed %d: covered %d, ambiguous pixels %d; vs float64: boxes with another area %d, visible %d (largest %d, %d)"
          % (seed, c["covered"], c["ambiguous_pixels"], (da > 0).sum(), (dv > 0).sum(), da.max(), dv.max()))
    assert (da <= c["ambiguous"]).all() and (dv <= c["ambiguous"]).all()
    assert c["ambiguous_pixels"] <= AMBIGUOUS_CAP * c["covered"]
    assert visible[c["row_tie_b"]] == 0 and visible[c["row_tie_a"]] == c["visible"][c["row_tie_a"]]
    # (a) the per-image kernel of the same library
    area1, visible1 = _per_image(dev, c)
    ea, ev = np.abs(area - area1), np.abs(visible - visible1)
    print("seed %d: vs per-image kernel: boxes with another area %d, visible %d" % (seed, (ea > 0).sum(), (ev > 0).sum()))
    if exact:
        assert np.array_equal(area, area1) and np.array_equal(visible, visible1)
    else:
        assert (ea <= c["ambiguous"]).all() and (ev <= c["ambiguous"]).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_visibility_ragged_emulated(emu_lib, seed):
    _run_case("cpu", seed, exact=True)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_visibility_ragged_gpu(hip_lib, seed):
    _run_case("cuda", seed, exact=False)


# ---- (c) images keep to themselves; empty inputs -----------------------------------------------------------------------------------

def _select(c, images):
    """the scene made of `images` (indices into the case, in this order)"""
    off = c["box_off"]
    rows = np.concatenate([np.arange(off[i], off[i + 1]) for i in images] + [np.zeros(0, np.int64)]).astype(np.int64)
    counts = [int(off[i + 1] - off[i]) for i in images]
    sub = dict(box3d=c["box3d"][rows], R=c["R"][rows], box_off=np.concatenate(([0], np.cumsum(counts))).astype(np.int32),
               K=c["K"][list(images)].reshape(-1, 9), size=c["size"][list(images)].reshape(-1, 2))
    return sub, rows


def _run_images(dev):
    from omni3d_amd.kernels import annotate
    c = _case(SEEDS[0])
    small = [i for i in range(len(SIZES)) if SIZES[i][0] < 100]
    whole, rows = _select(c, small)
    area, visible = [o.cpu().numpy() for o in annotate.visibility_ragged(*_t(whole, dev), zplane=ZPLANE)]
    pos = {int(r): k for k, r in enumerate(rows)}
    # an image alone, boxes or not, gives the rows it has in the whole scene
    for i in small:
        one, r = _select(c, [i])
        a1, v1 = [o.cpu().numpy() for o in annotate.visibility_ragged(*_t(one, dev), zplane=ZPLANE)]
        at = [pos[int(x)] for x in r]
        assert a1.shape == (len(r),) and np.array_equal(a1, area[at]) and np.array_equal(v1, visible[at])
    # permuted images: permuted counters
    perm = [small[k] for k in (3, 0, 5, 2, 4, 1)]
    mixed, r = _select(c, perm)
    a2, v2 = [o.cpu().numpy() for o in annotate.visibility_ragged(*_t(mixed, dev), zplane=ZPLANE)]
    at = [pos[int(x)] for x in r]
    assert np.array_equal(a2, area[at]) and np.array_equal(v2, visible[at])
    # no image, no box
    for images in ([], [3], [3, 3]):
        sub, _ = _select(c, images)
        a0, v0 = annotate.visibility_ragged(*_t(sub, dev), zplane=ZPLANE)
        assert tuple(a0.shape) == (0,) and tuple(v0.shape) == (0,) and a0.dtype == torch.int32


def test_images_keep_to_themselves_emulated(emu_lib):
    _run_images("cpu")


@pytest.mark.gpu
def test_images_keep_to_themselves_gpu(hip_lib):
    _run_images("cuda")
