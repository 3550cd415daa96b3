"""omni_fill_shapes (csrc/shapes.hip) against a float64 reference written here from the definition, by a method the kernel does not
use: the kernel decides on which side of an edge a pixel lies from the sign of the edge function (a cross product, no division)
and combines four such decisions with XOR; the reference computes where every edge meets the pixel's scan line (a division) and
counts the meeting points to the right of the pixel -- the crossing number, odd: inside.  Rings compare the float64 distance with
the two radii.  Shapes are applied in list order with out = floor(v * blend + (1 - blend) * c) in float64.

The images must equal the reference exactly outside the unsure pixels: those whose centre lies, in the float64 reference, within
1e-3 px of an edge of a quadrilateral or of a radius of a ring.  Unsure pixels are at most 0.5 % of the pixels a case paints
(asserted; met by the chosen coordinates with the reference alone)."""
import functools

import numpy as np
import pytest
import torch

EDGE_TOL, UNSURE_CAP = 1e-3, 0.005
VIEWS = ((64, 80), (50, 70))          # (H, W); the second leaves partial tiles on both edges


def quad(pts, blend, color):
    return [0.0] + [float(v) for p in pts for v in p] + [float(blend)] + [float(c) for c in color]


def ring(cx, cy, outer, inner, blend, color):
    return [1.0, float(cx), float(cy), float(outer), float(inner), 0.0, 0.0, 0.0, 0.0, float(blend)] + [float(c) for c in color]


CONVEX = [(10.3, 8.2), (40.7, 12.4), (35.2, 40.6), (8.9, 30.1)]
CONCAVE = [(50.3, 5.2), (62.4, 20.9), (75.6, 6.3), (63.2, 45.8)]                  # (62.4, 20.9) is a reflex vertex
BOWTIE = [(10.2, 35.3), (40.6, 60.7), (40.9, 36.2), (9.8, 58.4)]                  # edges 0-1 and 2-3 cross
PARTLY = [(60.3, 50.2), (95.7, 45.1), (99.2, 80.3), (55.4, 70.6)]
OUTSIDE = [(-30.2, -20.3), (-5.1, -25.7), (-3.3, -2.2), (-28.4, -4.6)]
OVER_A = quad([(20.3, 15.2), (50.6, 17.4), (48.2, 44.7), (18.7, 41.3)], 0.5, (250, 10, 20))
OVER_B = ring(45.3, 30.6, 12.7, 0.0, 0.5, (10, 240, 130))


def _random_shapes(n, seed):
    rs = np.random.RandomState(seed)
    rows = []
    for k in range(n):
        cx, cy = rs.uniform(-6, 86), rs.uniform(-6, 70)
        blend = float(rs.choice([0.0, 0.25, 0.33, 0.5, 0.8]))
        color = rs.randint(0, 256, 3)
        if k % 3 == 2:
            outer = rs.uniform(1.5, 6.0)
            rows.append(ring(cx, cy, outer, rs.choice([0.0, max(outer - 1.3, 0.0)]), blend, color))
        else:
            ang = np.sort(rs.uniform(0, 2 * np.pi, 4))
            if k % 3 == 1:
                ang = ang[[0, 2, 1, 3]]                                           # folded
            rad = rs.uniform(2.0, 7.0, 4)
            rows.append(quad([(cx + r * np.cos(a), cy + r * np.sin(a)) for r, a in zip(rad, ang)], blend, color))
    return rows


@functools.lru_cache(maxsize=None)
def _sets():
    hand = [quad(CONVEX, 0.5, (200, 30, 90)), quad(CONCAVE, 0.33, (20, 220, 60)), quad(BOWTIE, 0.5, (0, 0, 255)),
            quad(PARTLY, 0.25, (255, 255, 0)), quad(OUTSIDE, 0.5, (1, 2, 3)), ring(30.3, 25.6, 9.7, 0.0, 0.5, (90, 10, 200)),
            ring(55.4, 30.7, 12.23, 11.23, 0.0, (255, 128, 0)), ring(20.6, 48.3, 8.3, 5.3, 0.33, (0, 200, 200)),
            ring(33.3, 33.7, 0.0, 0.0, 0.0, (9, 9, 9))]
    many = _random_shapes(150, 4)
    nan_row = quad([(5.2, 5.3), (float("nan"), 9.1), (30.4, 31.2), (4.1, 28.3)], 0.0, (255, 0, 255))
    inf_row = ring(40.2, 20.3, float("inf"), 0.0, 0.0, (255, 0, 255))
    sets = {"convex": [hand[0]], "concave": [hand[1]], "bowtie": [hand[2]], "partly": [hand[3]], "outside": [hand[4]],
            "disc": [hand[5]], "ring1": [hand[6]], "ring3": [hand[7]], "radius0": [hand[8]],
            "over_ab": [OVER_A, OVER_B], "over_ba": [OVER_B, OVER_A],
            "many": hand[:4] + many[:75] + hand[4:] + many[75:] + [OVER_A, OVER_B],
            "nan": [hand[0], nan_row, inf_row, hand[5]], "without_nan": [hand[0], hand[5]], "empty": []}
    for blend in (0.0, 0.5, 0.33, 1.0):
        sets["blend_%g" % blend] = [quad(CONVEX, blend, (200, 30, 90)), ring(30.3, 25.6, 9.7, 0.0, blend, (90, 10, 200))]
    return sets


def _segment_distance(xs, ys, a, b):
    e = b - a
    l2 = float(e @ e)
    s = np.clip(((xs - a[0]) * e[0] + (ys - a[1]) * e[1]) / l2, 0.0, 1.0) if l2 > 0 else np.zeros_like(xs)
    return np.hypot(xs - a[0] - s * e[0], ys - a[1] - s * e[1])


def _image(H, W):
    return np.random.RandomState(17).randint(0, 256, size=(3, H, W)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _reference(name, H, W):
    """-> (image after the shapes, covered (H,W) bool, unsure (H,W) bool); computed once, never written to"""
    rows = np.asarray(_sets()[name], np.float32).reshape(-1, 13).astype(np.float64)
    out = _image(H, W)
    ys, xs = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    covered, unsure = np.zeros((H, W), bool), np.zeros((H, W), bool)
    for row in rows:
        if not np.isfinite(row).all():
            continue
        if row[0] == 0.0:
            pts = row[1:9].reshape(4, 2)
            count = np.zeros((H, W), np.int64)
            for k in range(4):
                a, b = pts[k], pts[(k + 1) % 4]
                unsure |= _segment_distance(xs, ys, a, b) <= EDGE_TOL
                if a[1] == b[1]:
                    continue                                                      # along the scan line: never crossed
                spans = (a[1] > ys) != (b[1] > ys)
                meet = a[0] + (ys - a[1]) * (b[0] - a[0]) / (b[1] - a[1])
                count += spans & (xs < meet)
            inside = count % 2 == 1
        else:
            dist = np.hypot(xs - row[1], ys - row[2])
            inside = (dist <= row[3]) & (dist >= row[4])
            unsure |= np.abs(dist - row[3]) <= EDGE_TOL
            if row[4] > 0:
                unsure |= np.abs(dist - row[4]) <= EDGE_TOL
        covered |= inside
        for ch in range(3):
            mixed = np.floor(out[ch].astype(np.float64) * row[9] + (1.0 - row[9]) * row[10 + ch])
            out[ch][inside] = mixed[inside].astype(np.uint8)
    for a in (out, covered, unsure):
        a.setflags(write=False)
    return out, covered, unsure


CASES = [(name, H, W) for (H, W) in VIEWS for name in sorted(_sets())]
PAINT_NOTHING = ("outside", "radius0", "empty")


@pytest.mark.parametrize("name,H,W", CASES)
def test_unsure_pixels_stay_under_the_cap(name, H, W):
    """a condition on the chosen coordinates, checked with the reference alone"""
    _, covered, unsure = _reference(name, H, W)
    assert unsure.sum() <= UNSURE_CAP * covered.sum(), (int(unsure.sum()), int(covered.sum()))
    assert (covered.sum() == 0) == (name in PAINT_NOTHING)


def test_reference_follows_even_odd_and_list_order():
    H, W = VIEWS[0]
    _, covered, _ = _reference("bowtie", H, W)
    assert covered[45, 15] and covered[45, 36] and not covered[38, 25] and not covered[56, 25]      # the two lobes, not the notches
    ab, ba, base = _reference("over_ab", H, W)[0], _reference("over_ba", H, W)[0], _image(H, W)
    y, x = 30, 42                                                                                   # inside both shapes
    one = lambda v, c: np.floor(v * 0.5 + 0.5 * c)                                                  # noqa: E731
    assert [one(one(float(base[c, y, x]), OVER_A[10 + c]), OVER_B[10 + c]) for c in range(3)] == ab[:, y, x].tolist()
    assert [one(one(float(base[c, y, x]), OVER_B[10 + c]), OVER_A[10 + c]) for c in range(3)] == ba[:, y, x].tolist()
    assert (ab != ba).any()


def _run(dev, name, H, W):
    from omni3d_amd.kernels import render
    want, covered, unsure = _reference(name, H, W)
    assert unsure.sum() <= UNSURE_CAP * covered.sum()
    shapes = torch.tensor(np.asarray(_sets()[name], np.float32).reshape(-1, 13)).to(dev)
    base = _image(H, W)
    got = [render.fill_shapes(torch.from_numpy(base.copy()).to(dev), shapes) for _ in range(2)]
    assert torch.equal(got[0], got[1])                                        # two runs give the same bits
    got = got[0].cpu().numpy()
    wrong = (got != want).any(0) & ~unsure
    print("fill %s %dx%d: %d covered, %d unsure, %d wrong" % (name, H, W, covered.sum(), unsure.sum(), wrong.sum()))
    assert not wrong.any(), np.argwhere(wrong)[:5].tolist()
    assert np.array_equal(got[:, ~covered & ~unsure], base[:, ~covered & ~unsure])      # uncovered pixels are not touched
    return got


def _run_all(dev):
    for H, W in VIEWS:
        got = {name: _run(dev, name, H, W) for name in sorted(_sets())}
        base = _image(H, W)
        for name in PAINT_NOTHING + ("blend_1",):
            assert np.array_equal(got[name], base), name
        assert np.array_equal(got["nan"], got["without_nan"])                 # rows that are not finite cover nothing
        assert (got["over_ab"] != got["over_ba"]).any()                       # the list order shows
        assert (got["blend_0"] != got["blend_0.5"]).any() and (got["blend_0.33"] != got["blend_0.5"]).any()
    assert len(_sets()["many"]) > 128                                         # more than two LDS chunks


def test_fill_shapes_emulated(emu_lib):
    _run_all("cpu")


@pytest.mark.gpu
def test_fill_shapes_gpu(hip_lib):
    _run_all("cuda")
