"""csrc/bev_iou.hip (`kernels.bev`: omni_bev_footprint, omni_bev_iou_pairs) against tests/exact_bev.py, the float64 form of the
definition: footprint = convex hull of the corners projected along `up`, IoU of two footprints by clipping, 0 for an invalid box (a
non-finite vertex, footprint area <= 1e-8) and for disjoint bounding rectangles.

Every body runs under the host emulator and, marked `gpu`, on the device; the outputs are poisoned before each launch; the pair lists
have 1, 63, 64, 65 and 257 entries (one thread, the wave boundary, five workgroups with a tail) over up to 130 boxes per side, with
repeats and ragged groups.  Bounds: |iou - float64| <= 1e-5 absolute (the IoU3D bound of tests/test_iou3d.py), footprint area 1e-5
relative; the float32 form of the reference alone must stay within 1e-6 on the same pairs, which shows without any kernel that
the inputs sit well inside the bound.  Hull sizes: 6 for a generic rotation, exactly 4 for a yaw-only box under the default `up`
(the duplicated corners are bit-equal); for the tilted sets, whose corners nearly coincide, the size may differ between precisions
and only area and IoU are compared.  `boxgen.omni3d_like_pairs` makes 3 % of its detections degenerate here (a zero dimension: a plate
whose footprint is a parallelogram; or a skewed vertex): their hull size is compared with the float64 one instead of with 6.

Largest |iou - float64| over all random sets, kernel | float32 reference, printed by every run under `-s`:
    host emulator   3.04e-07 | 3.04e-07
    MI355X          3.04e-07 | 3.04e-07
"""
import functools

import numpy as np
import pytest
import torch

import exact_bev
from omni3d_amd import boxgen

IOU_TOL, AREA_RTOL, REF32_TOL = 1e-5, 1e-5, 1e-6
POISON = -77
PAIR_COUNTS = (1, 63, 64, 65, 257)
N_BOXES = 130
TILTS = (1e-2, 1e-3, 1e-5, 1e-7)
UP_GENERIC = np.array([0.31, -0.87, 0.42]) / np.linalg.norm([0.31, -0.87, 0.42])
YAW_GENERIC = 0.6435


def _ry(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def _rx(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def _frame(up):
    """rotation whose columns are (e1, -up, e2): a box built with it stands upright with respect to `up`"""
    e1, e2 = exact_bev.plane_basis(up)
    u = np.asarray(up, np.float64) / np.linalg.norm(up)
    return np.stack([e1, -u, e2], axis=1)


def _upright(center_plane, height_pos, dims, yaw, up=exact_bev.UP):
    """one box upright with respect to `up`: centre (a, b) in the (e1, e2) plane, `height_pos` along -up, dims (l, h, w), yaw"""
    F = _frame(up)
    c = F @ np.array([center_plane[0], height_pos, center_plane[1]])
    return boxgen.corners(c[None], np.asarray(dims, np.float64)[None], (F @ _ry(yaw))[None])[0]


def _index_lists(rng, n):
    """257 pairs over n boxes per side: the matched pairs (i, i), three ragged (detections x ground truths) groups, random pairs
    with repeats"""
    i1, i2 = [np.arange(n)], [np.arange(n)]
    for d0, nd, g0, ng in ((3, 3, 2, 4), (20, 5, 21, 2), (40, 2, 38, 6)):
        i1.append(d0 + np.repeat(np.arange(nd), ng)), i2.append(g0 + np.tile(np.arange(ng), nd))
    rest = 257 - sum(len(a) for a in i1)
    r = rng.integers(n, size=rest)
    i1.append(r), i2.append(np.clip(r + rng.integers(-1, 2, size=rest), 0, n - 1))
    return np.concatenate(i1).astype(np.int32), np.concatenate(i2).astype(np.int32)


def _yaw_pairs(rng, n, tilt=0.0):
    """yaw-only boxes out to z = 80, x = +-20, dimensions 0.05 .. 20; 70 % of the second set are jittered copies of the first.
    tilt: every box is also turned about x by this angle (nearly coincident top and bottom corners)"""
    def one(c, d, yaw):
        R = np.stack([_rx(tilt) @ _ry(a) for a in yaw])
        return boxgen.corners(c, d, R)
    c = np.stack([rng.uniform(-20, 20, n), rng.uniform(-2, 2, n), rng.uniform(2, 80, n)], 1)
    d = np.exp(rng.uniform(np.log(0.05), np.log(20.0), size=(n, 3)))
    yaw = rng.uniform(-np.pi, np.pi, n)
    c2 = np.stack([rng.uniform(-20, 20, n), rng.uniform(-2, 2, n), rng.uniform(2, 80, n)], 1)
    d2 = np.exp(rng.uniform(np.log(0.05), np.log(20.0), size=(n, 3)))
    yaw2 = rng.uniform(-np.pi, np.pi, n)
    ov = rng.uniform(size=n) < 0.7
    c2[ov] = c[ov] + rng.normal(scale=0.3, size=(ov.sum(), 3)) * d[ov]
    d2[ov] = d[ov] * rng.uniform(0.7, 1.3, size=(ov.sum(), 3))
    yaw2[ov] = yaw[ov] + rng.normal(scale=0.2, size=ov.sum())
    return one(c, d, yaw), one(c2, d2, yaw2)


@functools.lru_cache(maxsize=None)
def _random_set(name):
    """boxes, pair lists and the float64 / float32 references of one random set, computed once and never written to"""
    rng = np.random.default_rng({"omni": 11, "yaw": 12}.get(name, 13))
    if name == "omni":
        dt, gt, deg = boxgen.omni3d_like_pairs(rng, N_BOXES, degenerate_frac=0.03)
    else:
        dt, gt = _yaw_pairs(rng, N_BOXES, 0.0 if name == "yaw" else float(name))
        deg = np.zeros(N_BOXES, bool)
    idx1, idx2 = _index_lists(rng, N_BOXES)
    f64 = [exact_bev.footprints(b, dtype=np.float64) for b in (dt, gt)]
    f32 = [exact_bev.footprints(b, dtype=np.float32) for b in (dt, gt)]
    out = dict(dt=dt, gt=gt, deg=deg, idx1=idx1, idx2=idx2,
               count=[np.array([len(h) for h, _ in f], np.int32) for f in f64], area=[np.array([a for _, a in f], np.float64) for f in f64],
               iou=exact_bev.bev_iou_pairs(f64[0], f64[1], idx1, idx2, np.float64),
               iou32=exact_bev.bev_iou_pairs(f32[0], f32[1], idx1, idx2, np.float32).astype(np.float64))
    for v in out.values():
        v.setflags(write=False) if isinstance(v, np.ndarray) else [a.setflags(write=False) for a in v]
    return out


RANDOM_SETS = ("omni", "yaw") + tuple(repr(t) for t in TILTS)


@pytest.mark.parametrize("name", RANDOM_SETS)
def test_reference_alone_meets_the_conditions(name):
    """no kernel: the float32 form of the reference is within 1e-6 of the float64 one on the pairs the kernel tests use, the sets
    have overlapping, disjoint and (omni) degenerate members, and the hull sizes are what the module docstring says"""
    s = _random_set(name)
    e = float(np.abs(s["iou32"] - s["iou"]).max())
    print("%s: |ref32 - fp64| %.2e" % (name, e))
    assert e <= REF32_TOL, e
    assert (s["iou"] > 0.2).sum() > 40 and (s["iou"] == 0).sum() > 20 and s["iou"].max() <= 1.0
    if name == "omni":
        assert s["deg"].sum() >= 2 and (s["count"][0][~s["deg"]] == 6).all() and (s["count"][1] == 6).all()
    elif name == "yaw":
        assert (s["count"][0] == 4).all() and (s["count"][1] == 4).all()
    assert len(s["idx1"]) == 257 and len(np.unique(s["idx1"])) < 257 and s["idx1"].max() == N_BOXES - 1


def test_local_origin_is_what_keeps_float32_inside_the_bound():
    """no kernel: the same float32 steps in absolute coordinates lose well over an order of magnitude on the far set and MISS the
    bound the kernel is held to there (1.6e-5 against 3.0e-7), so the far set does catch a kernel that skips the local origin"""
    s = _random_set("yaw")
    f32 = [exact_bev.footprints(b, dtype=np.float32) for b in (s["dt"], s["gt"])]
    absolute = exact_bev.bev_iou_pairs(f32[0], f32[1], s["idx1"], s["idx2"], np.float32, local_origin=False).astype(np.float64)
    worst = np.abs(absolute - s["iou"]).max()
    assert worst > 20 * np.abs(s["iou32"] - s["iou"]).max() and worst > IOU_TOL


def _poison(monkeypatch):
    from omni3d_amd.kernels import bev
    monkeypatch.setattr(bev, "_empty", lambda shape, dtype, like: torch.full(shape, POISON, dtype=dtype, device=like.device))
    return bev


def _bits(t):
    return t.cpu().contiguous().view(torch.int32)


def _check_polygons(poly, count, area, want_area):
    """counter-clockwise, strictly convex in float32 terms, zeros behind the count, area = the reference's"""
    for n in range(len(count)):
        k = int(count[n])
        assert (poly[n, k:] == 0).all()
        if k == 0:
            assert area[n] == 0 and want_area[n] == 0
            continue
        assert 3 <= k <= 8
        h = poly[n, :k].astype(np.float64)
        a, b, c = h, np.roll(h, -1, 0), np.roll(h, -2, 0)
        turn = (b[:, 0] - a[:, 0]) * (c[:, 1] - b[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - b[:, 0])
        assert (turn > -1e-6 * max(want_area[n], 1e-3)).all(), (n, turn)
        assert abs(area[n] - want_area[n]) <= AREA_RTOL * want_area[n], (n, area[n], want_area[n])


def _run_random(dev, name, monkeypatch):
    bev = _poison(monkeypatch)
    s = _random_set(name)
    dt, gt = torch.from_numpy(np.array(s["dt"])).to(dev), torch.from_numpy(np.array(s["gt"])).to(dev)
    idx1, idx2 = torch.from_numpy(np.array(s["idx1"])).to(dev), torch.from_numpy(np.array(s["idx2"])).to(dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    fps = [bev.bev_footprints(dt, counts=bad), bev.bev_footprints(gt)]
    again = bev.bev_footprints(dt)
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(fps[0], again))
    assert int(bad) == int((fps[0][1] == 0).sum()) == int((s["count"][0] == 0).sum())
    for side, fp in enumerate(fps):
        poly, count, area = [t.cpu().numpy() for t in fp]
        assert poly.shape == (N_BOXES, 8, 2) and count.shape == (N_BOXES,) and area.shape == (N_BOXES,)
        _check_polygons(poly, count, area, s["area"][side])
        if name in ("omni", "yaw"):
            assert np.array_equal(count, s["count"][side]), np.flatnonzero(count != s["count"][side])
        else:
            assert ((count >= 4) & (count <= 8)).all()
    worst = 0.0
    for P in PAIR_COUNTS:
        a, b = bev.bev_iou_pairs(fps[0], fps[1], idx1[:P], idx2[:P]), bev.bev_iou_pairs(fps[0], fps[1], idx1[:P], idx2[:P])
        assert a.shape == (P,) and torch.equal(_bits(a), _bits(b))                            # two launches are bit-identical
        got, want = a.cpu().numpy().astype(np.float64), s["iou"][:P]
        assert np.isfinite(got).all() and got.min() >= 0 and got.max() <= 1
        worst = max(worst, float(np.abs(got - want).max()))
        inv = (s["count"][0][s["idx1"][:P]] == 0) | (s["count"][1][s["idx2"][:P]] == 0)
        assert (got[inv] == 0).all()
    print("%s: |hip - fp64| %.2e  |ref32 - fp64| %.2e over %d pairs" % (name, worst, np.abs(s["iou32"] - s["iou"]).max(), 257))
    assert worst <= IOU_TOL, worst


@pytest.mark.parametrize("name", RANDOM_SETS)
def test_random_pairs_emulated(emu_lib, monkeypatch, name):
    _run_random("cpu", name, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", RANDOM_SETS)
def test_random_pairs_gpu(hip_lib, monkeypatch, name):
    _run_random("cuda", name, monkeypatch)


def _closed_forms(up, yaw):
    """(box a, box b, IoU in closed form, exact) for footprints l x w = 4 x 2 turned by `yaw`, upright with respect to `up`"""
    c, s = np.cos(yaw), np.sin(yaw)
    at = lambda u, v: (3.0 + c * u + s * v, 30.0 - s * u + c * v)       # noqa: E731  (u, v) along the footprint's own axes
    d = (4.0, 1.5, 2.0)
    box = lambda u, v, dims=d, h=0.3: _upright(at(u, v), h, dims, yaw, up)      # noqa: E731
    return [
        (box(0, 0), box(0, 0), 1.0, False),                                       # identical
        (box(0, 0), box(0, 0, (4.0, 1.5, 2.0), -0.7), 1.0, False),               # the same footprint at another height
        (box(0, 0), box(0, 0, (2.0, 0.75, 1.0)), 0.25, False),                    # contains a copy scaled by 1/2
        (box(0, 0, (2.8, 3.0, 1.4)), box(0, 0), 0.49, False),                     # is contained in a copy scaled by 1/0.7
        (box(0, 0), box(1.0, 0.5), 4.5 / 11.5, False),                            # offset by (1, 0.5): 3 x 1.5 in common
        (box(0, 0), box(4.0, 0), 0.0, False),                                     # share one edge only
        (box(0, 0), box(0, 2.0), 0.0, False),
        (box(0, 0), box(40.0, 35.0), 0.0, True),                                  # bounding rectangles disjoint: exactly 0
    ]


def _run_closed_forms(dev, monkeypatch):
    bev = _poison(monkeypatch)
    for up, yaw in ((exact_bev.UP, 0.0), (exact_bev.UP, YAW_GENERIC), (UP_GENERIC, YAW_GENERIC)):
        cases = _closed_forms(up, yaw)
        a = torch.from_numpy(np.stack([c[0] for c in cases])).to(dev)
        b = torch.from_numpy(np.stack([c[1] for c in cases])).to(dev)
        fa, fb = bev.bev_footprints(a, up=up), bev.bev_footprints(b, up=up)
        if up is exact_bev.UP:                                     # bit-equal top and bottom corners: the familiar rotated rectangle
            assert (fa[1] == 4).all() and (fb[1] == 4).all()
        assert abs(float(fa[2][0]) - 8.0) <= 8.0 * AREA_RTOL and abs(float(fb[2][2]) - 2.0) <= 2.0 * AREA_RTOL
        n = len(cases)
        idx = torch.arange(n, dtype=torch.int32, device=dev)
        got = bev.bev_iou_pairs(fa, fb, idx, idx).cpu().numpy()
        back = bev.bev_iou_pairs(fb, fa, idx, idx).cpu().numpy()
        for k, (box1, box2, want, exact) in enumerate(cases):
            ref = float(exact_bev.bev_iou(box1, box2, up=up))
            assert abs(ref - want) <= 1e-6, (k, ref, want)                                    # the reference against the closed form
            for v in (got[k], back[k]):
                assert abs(v - want) <= IOU_TOL, (up, yaw, k, v, want)
                assert not exact or v == 0.0


def test_closed_forms_emulated(emu_lib, monkeypatch):
    _run_closed_forms("cpu", monkeypatch)


@pytest.mark.gpu
def test_closed_forms_gpu(hip_lib, monkeypatch):
    _run_closed_forms("cuda", monkeypatch)


def _special_boxes():
    """rows: 0 a plain upright box, 1 the same with a NaN vertex, 2 upright with one horizontal dimension 0 (footprint = a segment),
    3 a zero-thickness plate at a generic rotation (a proper footprint), 4 a copy of row 0 moved a little"""
    R = boxgen.rand_rot(np.random.default_rng(5), 1)
    plain = _upright((1.0, 20.0), 0.0, (3.0, 1.5, 2.0), 0.4)
    nan = plain.copy()
    nan[5, 1] = np.nan
    segment = _upright((1.0, 20.0), 0.0, (0.0, 1.5, 2.0), 0.4)
    plate = boxgen.corners(np.array([[1.0, 0.5, 20.0]]), np.array([[3.0, 0.0, 2.0]]), R)[0]
    moved = _upright((1.4, 20.3), 0.1, (3.0, 1.5, 2.0), 0.5)
    return np.stack([plain, nan, segment, plate, moved]).astype(np.float32)


def _run_invalid(dev, monkeypatch):
    bev = _poison(monkeypatch)
    boxes = _special_boxes()
    want = [exact_bev.footprint(b) for b in boxes]
    assert [len(h) > 0 for h, _ in want] == [True, False, False, True, True]
    t = torch.from_numpy(boxes).to(dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    poly, count, area = bev.bev_footprints(t, counts=bad)
    assert int(bad) == 2
    assert count.tolist()[:3] == [4, 0, 0] and count[3] >= 4 and count[4] == 4
    assert (poly[1:3] == 0).all() and (area[1:3] == 0).all()
    _check_polygons(poly.cpu().numpy(), count.cpu().numpy(), area.cpu().numpy(), np.array([float(a) for _, a in want]))
    iou = bev.bev_overlap(t, t).cpu().numpy()
    assert np.isfinite(iou).all()
    assert (iou[1:3] == 0).all() and (iou[:, 1:3] == 0).all()                                 # on either side, exactly
    for i in (0, 3, 4):
        for j in (0, 3, 4):
            assert abs(iou[i, j] - float(exact_bev.iou_footprints(want[i], want[j]))) <= IOU_TOL
    assert iou[0, 4] > 0.3 and iou[0, 3] > 0.05


def test_invalid_boxes_emulated(emu_lib, monkeypatch):
    _run_invalid("cpu", monkeypatch)


@pytest.mark.gpu
def test_invalid_boxes_gpu(hip_lib, monkeypatch):
    _run_invalid("cuda", monkeypatch)


def _run_overlap_matrix(dev, monkeypatch):
    """bev_overlap is symmetric under swapping its arguments up to transposition (to the tolerance: the local origin and the
    clipped polygon change sides), its diagonal on valid boxes is 1 within tolerance; empty inputs launch nothing"""
    bev = _poison(monkeypatch)
    s = _random_set("omni")
    a, b = torch.from_numpy(np.array(s["dt"][:23])).to(dev), torch.from_numpy(np.array(s["gt"][:9])).to(dev)
    ab, ba = bev.bev_overlap(a, b).cpu().numpy(), bev.bev_overlap(b, a).cpu().numpy()
    assert ab.shape == (23, 9) and ba.shape == (9, 23)
    assert np.abs(ab - ba.T).max() <= IOU_TOL and np.array_equal(ab == 0, ba.T == 0)
    aa = bev.bev_overlap(a, a).cpu().numpy()
    valid = s["count"][0][:23] > 0
    assert np.abs(np.diag(aa)[valid] - 1.0).max() <= IOU_TOL and (np.diag(aa)[~valid] == 0).all()
    for n, m in ((0, 4), (4, 0), (0, 0)):
        assert bev.bev_overlap(a[:n], b[:m]).shape == (n, m)
    fp = bev.bev_footprints(a)
    none = torch.zeros(0, dtype=torch.int32, device=dev)
    assert bev.bev_iou_pairs(fp, fp, none, none).shape == (0,)
    # an index outside its set reads nothing and gives 0
    out = bev.bev_iou_pairs(fp, fp, torch.tensor([0, 23, -1, 2], dtype=torch.int32, device=dev), torch.tensor([0, 0, 0, 99], dtype=torch.int32, device=dev))
    assert out.tolist()[1:] == [0.0, 0.0, 0.0] and abs(float(out[0]) - 1.0) <= IOU_TOL


def test_overlap_matrix_emulated(emu_lib, monkeypatch):
    _run_overlap_matrix("cpu", monkeypatch)


@pytest.mark.gpu
def test_overlap_matrix_gpu(hip_lib, monkeypatch):
    _run_overlap_matrix("cuda", monkeypatch)


def _argument_errors(L, dev):
    from omni3d_amd import lib
    from omni3d_amd.kernels import bev
    b = torch.from_numpy(boxgen.random_boxes(np.random.default_rng(0), 6)).to(dev)
    fp = bev.bev_footprints(b)
    i = torch.arange(6, dtype=torch.int32, device=dev)
    for bad in (b[:, :7], b.double(), b.view(6, 24), b.transpose(1, 2).contiguous(), b[::2]):
        with pytest.raises(ValueError):
            bev.bev_footprints(bad)
    for kw in (dict(up=(0.0, 0.0, 0.0)), dict(up=(0.0, np.nan, 1.0)), dict(up=(1.0, 0.0)), dict(eps_area=-1.0), dict(eps_area=np.nan),
               dict(counts=torch.zeros(1, device=dev)), dict(counts=torch.zeros(2, dtype=torch.int32, device=dev))):
        with pytest.raises(ValueError):
            bev.bev_footprints(b, **kw)
    for bad in ((fp[:2], fp, i, i), ((fp[0][:, :7], fp[1], fp[2]), fp, i, i), ((fp[0], fp[1].long(), fp[2]), fp, i, i),
                ((fp[0], fp[1], fp[2][:5]), fp, i, i), (fp, (fp[0].double(), fp[1], fp[2]), i, i), (fp, fp, i[:5], i), (fp, fp, i.float(), i),
                (fp, fp, i.view(2, 3), i.view(2, 3)), (fp, (fp[0], fp[1], fp[2].double()), i, i)):
        with pytest.raises(ValueError):
            bev.bev_iou_pairs(*bad)
    # the C entry points: the error status before anything touches the device, the outputs keep their poison
    outs = [torch.full(s, POISON, dtype=d, device=dev) for s, d in (((6, 8, 2), torch.float32), ((6,), torch.int32), ((6,), torch.float32))]
    iou = torch.full((6,), POISON, dtype=torch.float32, device=dev)
    P = lambda t: t.data_ptr()      # noqa: E731
    st = lib.stream_of(b)
    foot, pairs = L._fn["omni_bev_footprint"], L._fn["omni_bev_iou_pairs"]
    assert foot(P(b), -1, 1, 0, 0, 0, 0, 1, 1e-8, *map(P, outs), None, st) == 1
    assert foot(P(b), 6, 1, 0, 0, 0, 0, 1, -1.0, *map(P, outs), None, st) == 1
    assert foot(P(b), 6, 1, 0, 0, 0, 0, 1, float("nan"), *map(P, outs), None, st) == 1
    assert foot(P(b), 6, float("nan"), 0, 0, 0, 0, 1, 1e-8, *map(P, outs), None, st) == 1
    assert foot(P(b), 6, 1, 0, 0, 0, 0, 1, 1e-8, None, P(outs[1]), P(outs[2]), None, st) == 1
    assert foot(None, 0, 1, 0, 0, 0, 0, 1, 1e-8, None, None, None, None, st) == 0
    assert pairs(*map(P, fp), 6, *map(P, fp), 6, P(i), P(i), -1, P(iou), st) == 1
    assert pairs(*map(P, fp), -6, *map(P, fp), 6, P(i), P(i), 6, P(iou), st) == 1
    assert pairs(*map(P, fp), 6, *map(P, fp), 6, None, P(i), 6, P(iou), st) == 1
    assert pairs(*map(P, fp), 6, None, None, None, 6, P(i), P(i), 6, P(iou), st) == 1
    assert pairs(*map(P, fp), 6, *map(P, fp), 6, P(i), P(i), 6, None, st) == 1
    assert pairs(None, None, None, 0, None, None, None, 0, None, None, 0, None, st) == 0
    if dev == "cuda":
        torch.cuda.synchronize()
    assert all(bool((o == POISON).all()) for o in outs + [iou])


def test_argument_errors_emulated(emu_lib):
    _argument_errors(emu_lib, "cpu")


@pytest.mark.gpu
def test_argument_errors_gpu(hip_lib):
    _argument_errors(hip_lib, "cuda")
