"""csrc/cuboid_exact.h + csrc/iou3d_exact.hip (`kernels.iou3d`: cuboid_fit, iou_box3d_exact, iou_box3d_exact_pairs) against float64
references computed from the same float32 vertices.  The kernel is held to 1e-5 absolute on IoU, the project's IoU3D bound
(tests/test_bev_iou.py, tests/test_iou3d.py), on four kinds of input:

  H  hand-placed pairs with closed forms, in one generic frame (R0, T0): identical, shifted along one axis (four shared face
     planes), shifted along all three, concentric at half size, a half box sharing five face planes, A inside a large B of another
     rotation, touching faces (<= 1e-8), disjoint spheres (exactly 0), and three invalid boxes (a NaN vertex, a zero dimension, a
     vertex moved by 0.5): exactly 0 and counted.  The closed form is evaluated on the float64 parameters the vertices were rounded
     from.  Touching faces are held to 1e-8 on dyadic coordinates, which float32 holds exactly (upright, and turned by a quarter
     turn).  In the generic frame the rounded vertices no longer touch: the two fitted faces tilt against each other by the 1e-6 of
     float32 granularity at z = 40, and the IoU of the cuboids the kernel is given is 2e-9 .. 8e-8 along the three axes (measured,
     the float64 fit says the same: the planes' offsets agree to 1e-13, the wedge between them is real).  Those three pairs are held
     to the closed form 0 with the general 1e-5, like every other pair of H.
  Y  300 yaw-only near-duplicates (centres x +-20, z 3..80, dimensions 0.5..5, copies jittered by 0.15, relative yaw drawn from
     {0, 1e-6, 1e-4, 1e-3, 0.01, 0.03, 0.1} rad, half of them with equal height and y centre): reference = footprint intersection
     of tests/exact_bev.py x the overlap of the y extents.
  T  150 jittered copies turned 0.3 to 3 degrees about random axes: reference tests/exact_iou3d.py.
  G  400 `boxgen.omni3d_like_pairs(degenerate_frac=0)`: reference tests/exact_iou3d.py.

Y and T are what the evaluator's float32 pair algorithm (oracle/iou_box3d_oracle.c, no kernel involved) gets wrong: it must differ
from the reference by more than 1e-2 on at least one pair of each, which `test_references_alone` asserts on the CPU together with the
closed forms (1e-9) and the validity of every generated box.

Largest |iou - float64|, kernel | float32 pair algorithm, printed by every run under `-s`:
                    H (kernel)   Y                     T                     G
    host emulator   2.38e-07     7.16e-07 | 2.98e-01   5.98e-07 | 1.85e-01   1.41e-06 | 2.02e-01
    MI355X          2.38e-07     7.16e-07 | 2.98e-01   5.98e-07 | 1.85e-01   1.41e-06 | 2.02e-01
The float32 pair algorithm is off by more than 1e-2 on 14 pairs of Y, 19 of T and 2 of G.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import exact_bev
import exact_iou3d
from omni3d_amd import boxgen

IOU_TOL, SYM_TOL, TOUCH_TOL, GAP = 1e-5, 1e-6, 1e-8, 1e-2
EPS_DIM, FIT_TOL = 1e-8, 1e-3
POISON = -77
YAWS = (0.0, 1e-6, 1e-4, 1e-3, 0.01, 0.03, 0.1)
R0, T0 = boxgen.rand_rot(np.random.default_rng(7), 1)[0], np.array([3.0, -1.0, 40.0])      # the hand-placed boxes' common, generic frame
R1 = boxgen.rand_rot(np.random.default_rng(8), 1)[0]
D = np.array([2.0, 1.2, 1.6])


def _shift_for(iou):
    """the fraction f by which a box is shifted along all three of its axes to overlap its unshifted copy with this IoU"""
    r = 2.0 * iou / (1.0 + iou)                   # inter / volume = (1 - f)^3
    return 1.0 - r ** (1.0 / 3.0)


def _closed_form(a, b):
    (ca, da), (cb, db) = a, b
    ov = np.clip(np.minimum(ca + da / 2, cb + db / 2) - np.maximum(ca - da / 2, cb - db / 2), 0.0, None)
    inter = float(np.prod(ov))
    return inter / (float(np.prod(da)) + float(np.prod(db)) - inter)


def _frame_box(c, d, R=R0, T=T0):
    return boxgen.corners((R @ c + T)[None], np.asarray(d, np.float64)[None], R[None])[0]


def _ry(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def _axis_turn(axis, angle):
    k = axis / np.linalg.norm(axis)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


@functools.lru_cache(maxsize=None)
def _hand():
    """name -> (box1, box2, IoU in closed form, what is asserted: 'tol' | 'touch' | 'zero')"""
    z = np.zeros(3)
    f1, f3 = 0.3, _shift_for(0.27)
    ax0 = np.array([1.0, 0.0, 0.0])
    par = {
        "identical": ((z, D), (z, D), 1.0),
        "shift_one_axis": ((z, D), (f1 * D * ax0, D), (1.0 - f1) / (1.0 + f1)),
        "shift_three_axes": ((z, D), (f3 * D, D), 0.27),
        "concentric_half": ((z, D), (z, D / 2), 0.125),
        "half_box_five_planes": ((z, D), (-D * ax0 / 4, D * np.array([0.5, 1.0, 1.0])), 0.5),
    }
    out = {}
    for k, (a, b, want) in par.items():
        assert abs(_closed_form(a, b) - want) < 1e-9, k
        out[k] = (_frame_box(*a), _frame_box(*b), want, "tol")
    # A inside a large B of another rotation about the same centre: the volume ratio
    big = np.array([9.0, 8.0, 10.0])
    out["inside_rotated"] = (_frame_box(z, D), boxgen.corners((R0 @ z + T0)[None], big[None], R1[None])[0], float(np.prod(D) / np.prod(big)), "tol")
    # touching across one face, coordinates that float32 holds exactly: upright and turned by a quarter turn about y
    eye, quarter = np.eye(3), _ry(np.pi / 2).round()
    c = np.array([3.0, -1.0, 40.0])
    out["touching_x"] = (_frame_box(z, [2.0, 1.0, 1.5], eye, c), _frame_box(np.array([2.0, 0.25, 0.0]), [2.0, 1.0, 1.5], eye, c), 0.0, "touch")
    out["touching_z_quarter_turn"] = (_frame_box(z, [2.0, 1.0, 1.5], eye, c), _frame_box(np.array([0.25, 0.0, 1.75]), [2.0, 1.0, 1.5], quarter, c), 0.0, "touch")
    # the same in the generic frame: the rounded vertices no longer touch, the closed form 0 holds to the general tolerance only
    for ax in range(3):
        out["touching_generic_%d" % ax] = (_frame_box(z, D), _frame_box(D * np.eye(3)[ax], D), 0.0, "tol")
    out["disjoint_spheres"] = (_frame_box(z, D), _frame_box(np.array([12.0, 0.0, 0.0]), D), 0.0, "zero")
    return out


def _invalid_boxes():
    """rows 0..2 invalid (a NaN vertex, a zero dimension, `boxgen`'s skewed vertex), row 3 the plain box they were made from"""
    plain = _frame_box(np.zeros(3), D)
    nan, skew = plain.copy(), plain.copy()
    nan[5, 1] = np.nan
    skew[6] += np.float32(0.5)
    flat = _frame_box(np.zeros(3), D * np.array([1.0, 0.0, 1.0]))
    return np.stack([nan, flat, skew, plain]).astype(np.float32)


def fit64(box):
    """the fit of csrc/cuboid_exact.h in numpy float64 -> (centre, axes (3,3) rows, dims, valid)"""
    p = np.asarray(box, np.float64)
    if not np.isfinite(p).all():
        return np.zeros(3), np.zeros((3, 3)), np.zeros(3), False
    c = p.mean(0)
    e = np.stack([(p[1] - p[0] + p[2] - p[3] + p[5] - p[4] + p[6] - p[7]) / 4, (p[3] - p[0] + p[2] - p[1] + p[7] - p[4] + p[6] - p[5]) / 4,
                  (p[4] - p[0] + p[5] - p[1] + p[6] - p[2] + p[7] - p[3]) / 4])
    d = np.linalg.norm(e, axis=1)
    if not (d > EPS_DIM).all():
        return np.zeros(3), np.zeros((3, 3)), np.zeros(3), False
    x = e[0] / d[0]
    y = e[1] - (e[1] @ x) * x
    if not np.linalg.norm(y) > EPS_DIM:
        return np.zeros(3), np.zeros((3, 3)), np.zeros(3), False
    y = y / np.linalg.norm(y)
    zz = np.cross(x, y)
    zz = zz if zz @ e[2] >= 0 else -zz
    X = np.stack([x, y, zz])
    fitted = c + (boxgen.UNIT * d) @ X
    ok = np.linalg.norm(p - fitted, axis=1).max() <= FIT_TOL * d.max()
    return (c, X, d, True) if ok else (np.zeros(3), np.zeros((3, 3)), np.zeros(3), False)


def _yaw_set(rng, n=300):
    c = np.stack([rng.uniform(-20, 20, n), rng.uniform(-2, 2, n), rng.uniform(3, 80, n)], 1)
    d = rng.uniform(0.5, 5.0, size=(n, 3))
    yaw = rng.uniform(-np.pi, np.pi, n)
    c2 = c + rng.normal(scale=0.15, size=(n, 3)) * d
    d2 = d * rng.uniform(0.85, 1.15, size=(n, 3))
    yaw2 = yaw + rng.choice(YAWS, n) * rng.choice([-1.0, 1.0], n)
    same = np.arange(n) % 2 == 0                                   # equal height and y centre
    c2[same, 1], d2[same, 1] = c[same, 1], d[same, 1]
    return boxgen.corners(c, d, np.stack([_ry(a) for a in yaw])), boxgen.corners(c2, d2, np.stack([_ry(a) for a in yaw2]))


def _turned_set(rng, n=150):
    c = np.stack([rng.uniform(-5, 5, n), rng.uniform(-2, 2, n), rng.uniform(2, 40, n)], 1)
    d = rng.uniform(0.5, 5.0, size=(n, 3))
    R = boxgen.rand_rot(rng, n)
    c2 = c + rng.normal(scale=0.15, size=(n, 3)) * d
    d2 = d * rng.uniform(0.85, 1.15, size=(n, 3))
    R2 = np.stack([_axis_turn(rng.normal(size=3), np.radians(rng.uniform(0.3, 3.0))) @ R[k] for k in range(n)])
    return boxgen.corners(c, d, R), boxgen.corners(c2, d2, R2)


def _yaw_reference(b1, b2):
    """yaw-only boxes: footprint intersection (tests/exact_bev.py) x overlap of the y extents -> IoU3D in float64"""
    f1, f2 = exact_bev.footprint(b1), exact_bev.footprint(b2)
    r = float(exact_bev.iou_footprints(f1, f2))
    inter = r * (float(f1[1]) + float(f2[1])) / (1.0 + r)
    y1, y2 = b1[:, 1].astype(np.float64), b2[:, 1].astype(np.float64)
    oy = max(0.0, min(y1.max(), y2.max()) - max(y1.min(), y2.min()))
    v1, v2, v = float(f1[1]) * (y1.max() - y1.min()), float(f2[1]) * (y2.max() - y2.min()), inter * oy
    return v / (v1 + v2 - v)


@functools.lru_cache(maxsize=None)
def _set(name):
    """(boxes1, boxes2, float64 IoU of the matched pairs), computed once and never written to"""
    if name == "Y":
        a, b = _yaw_set(np.random.default_rng(21))
        ref = np.array([_yaw_reference(a[i], b[i]) for i in range(len(a))])
    elif name == "T":
        a, b = _turned_set(np.random.default_rng(22))
        ref = np.array([exact_iou3d.iou3d(a[i], b[i])[1] for i in range(len(a))])
    else:
        a, b, _ = boxgen.omni3d_like_pairs(np.random.default_rng(23), 400, degenerate_frac=0)
        ref = np.array([exact_iou3d.iou3d(a[i], b[i])[1] for i in range(len(a))])
    for v in (a, b, ref):
        v.setflags(write=False)
    return a, b, ref


def _oracle32(oracle_lib, a, b):
    """the float32 pair algorithm on the CPU (oracle/iou_box3d_oracle.c) for the matched pairs"""
    P = ctypes.c_void_p
    out, one = np.zeros(len(a), np.float64), np.zeros((1, 1), np.float32)
    for i in range(len(a)):
        x, y = np.ascontiguousarray(a[i:i + 1], np.float32), np.ascontiguousarray(b[i:i + 1], np.float32)
        oracle_lib.box3d_overlap_oracle(x.ctypes.data_as(P), 1, y.ctypes.data_as(P), 1, ctypes.c_float(1e-4), ctypes.c_float(1e-8), one.ctypes.data_as(P))
        out[i] = one[0, 0]
    return out


@functools.lru_cache(maxsize=None)
def _oracle_errors(name):
    """filled by test runs through `_gap`: |float32 pair algorithm - float64| of the set"""
    return {}


def _gap(oracle_lib, name):
    cache = _oracle_errors(name)
    if "e" not in cache:
        a, b, ref = _set(name)
        cache["e"] = np.abs(_oracle32(oracle_lib, a, b) - ref)
    return cache["e"]


def test_references_alone(oracle_lib):
    """no kernel: the closed forms hold to 1e-9 (asserted where `_hand` builds them), every generated box is a valid cuboid, the sets
    have overlapping members, and the evaluator's float32 algorithm is more than 1e-2 off on pairs of Y and of T"""
    hand = _hand()
    assert len(hand) == 12 and all(fit64(b)[3] for a, b, _, _ in hand.values()) and all(fit64(a)[3] for a, _, _, _ in hand.values())
    assert [fit64(b)[3] for b in _invalid_boxes()] == [False, False, False, True]
    for name, n in (("Y", 300), ("T", 150), ("G", 400)):
        a, b, ref = _set(name)
        assert len(a) == len(b) == len(ref) == n
        assert all(fit64(x)[3] for x in a) and all(fit64(x)[3] for x in b)
        assert np.isfinite(ref).all() and ref.min() >= 0 and ref.max() <= 1 and (ref > 0.2).sum() > n // 4
        e = _gap(oracle_lib, name)
        print("%s: float32 pair algorithm vs float64: worst %.2e, %d of %d pairs off by more than 1e-2" % (name, e.max(), (e > GAP).sum(), n))
        if name != "G":
            assert (e > GAP).sum() >= 1


def _poison(monkeypatch):
    from omni3d_amd.kernels import iou3d
    monkeypatch.setattr(iou3d, "_empty", lambda shape, dtype, like: torch.full(shape, POISON, dtype=dtype, device=like.device))
    return iou3d


def _bits(t):
    t = t.cpu().contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32)


def _matched(iou3d, dev, a, b):
    """matched pairs through the ragged form, twice (bit-identical), and swapped"""
    ta, tb = torch.from_numpy(np.array(a)).to(dev), torch.from_numpy(np.array(b)).to(dev)
    idx = torch.arange(len(a), dtype=torch.int32, device=dev)
    one, two = iou3d.iou_box3d_exact_pairs(ta, tb, idx, idx), iou3d.iou_box3d_exact_pairs(ta, tb, idx, idx)
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(one, two))                    # two launches are bit-identical
    back = iou3d.iou_box3d_exact_pairs(tb, ta, idx, idx)
    vol, iou, swapped = one[0].cpu().numpy().astype(np.float64), one[1].cpu().numpy().astype(np.float64), back[1].cpu().numpy().astype(np.float64)
    assert vol.shape == iou.shape == (len(a),)
    assert np.isfinite(vol).all() and np.isfinite(iou).all() and iou.min() >= 0 and iou.max() <= 1 and vol.min() >= 0     # written, never NaN
    assert np.abs(iou - swapped).max() <= SYM_TOL, np.abs(iou - swapped).max()
    return vol, iou


def _run_hand(dev, monkeypatch):
    iou3d = _poison(monkeypatch)
    hand = _hand()
    names = list(hand)
    _, iou = _matched(iou3d, dev, np.stack([hand[k][0] for k in names]), np.stack([hand[k][1] for k in names]))
    worst = 0.0
    for k, got in zip(names, iou):
        want, kind = hand[k][2], hand[k][3]
        if kind == "tol":
            worst = max(worst, abs(got - want))
            assert abs(got - want) <= IOU_TOL, (k, got, want)
        elif kind == "touch":
            assert got <= TOUCH_TOL, (k, got)
        else:
            assert got == 0.0, (k, got)
    vol = iou3d.iou_box3d_exact(torch.from_numpy(hand["identical"][0][None]).to(dev), torch.from_numpy(hand["inside_rotated"][1][None]).to(dev))[0]
    assert abs(float(vol) - float(np.prod(D))) <= 1e-5 * float(np.prod(D))                      # the intersection is A itself
    # invalid boxes: flagged, zeroed, counted once each, exactly 0 on either side
    boxes = torch.from_numpy(_invalid_boxes()).to(dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    centre, axes, dims, valid = iou3d.cuboid_fit(boxes, counts=bad)
    assert valid.tolist() == [0, 0, 0, 1] and int(bad) == 3
    assert (centre[:3] == 0).all() and (axes[:3] == 0).all() and (dims[:3] == 0).all()
    v, m = iou3d.iou_box3d_exact(boxes, boxes)
    for t in (v, m):
        t = t.cpu().numpy()
        assert np.isfinite(t).all() and (t[:3] == 0).all() and (t[:, :3] == 0).all()
    assert abs(float(m[3, 3]) - 1.0) <= IOU_TOL
    return worst


def _run_set(dev, name, monkeypatch, oracle_lib):
    iou3d = _poison(monkeypatch)
    a, b, ref = _set(name)
    _, iou = _matched(iou3d, dev, a, b)
    e = np.abs(iou - ref)
    o = _gap(oracle_lib, name)
    print("%s: |hip - fp64| %.2e  |float32 pair algorithm - fp64| %.2e over %d pairs" % (name, e.max(), o.max(), len(ref)))
    assert e.max() <= IOU_TOL, (int(e.argmax()), e.max())
    # the fit itself, against the same steps in numpy
    centre, axes, dims, valid = [t.cpu().numpy() for t in iou3d.cuboid_fit(torch.from_numpy(np.array(a[:70])).to(dev))]
    assert valid.all()
    for i in range(70):
        c, X, d, _ = fit64(a[i])
        assert np.abs(centre[i] - c).max() <= 1e-12 * 100 and np.abs(axes[i] - X).max() <= 1e-12 and np.abs(dims[i] - d).max() <= 1e-12 * 10


def _run_matrix(dev, monkeypatch):
    """the (N, M) form and the ragged form agree bit for bit; transposition is within 1e-6; empty inputs launch nothing; an index
    outside its set gives 0"""
    iou3d = _poison(monkeypatch)
    a, b, _ = _set("G")
    n, m = 23, 9
    ta, tb = torch.from_numpy(np.array(a[:n])).to(dev), torch.from_numpy(np.array(b[:m])).to(dev)
    vol, iou = iou3d.iou_box3d_exact(ta, tb)
    assert vol.shape == iou.shape == (n, m)
    i1 = torch.arange(n, dtype=torch.int64, device=dev).repeat_interleave(m)
    i2 = torch.arange(m, dtype=torch.int64, device=dev).repeat(n)
    pv, pi = iou3d.iou_box3d_exact_pairs(ta, tb, i1, i2)
    assert torch.equal(_bits(vol.reshape(-1)), _bits(pv)) and torch.equal(_bits(iou.reshape(-1)), _bits(pi))
    ba = iou3d.iou_box3d_exact(tb, ta)[1]
    assert float((iou - ba.T).abs().max()) <= SYM_TOL
    assert torch.equal(iou3d.box3d_overlap_exact(ta, tb), iou)
    aa = iou3d.iou_box3d_exact(ta, ta)[1].cpu().numpy()
    assert np.abs(np.diag(aa) - 1.0).max() <= IOU_TOL
    for p, q in ((0, 4), (4, 0), (0, 0)):
        v, r = iou3d.iou_box3d_exact(ta[:p], tb[:q])
        assert v.shape == (p, q) and r.shape == (p, q)
    none = torch.zeros(0, dtype=torch.int32, device=dev)
    assert iou3d.iou_box3d_exact_pairs(ta, tb, none, none)[1].shape == (0,)
    out = iou3d.iou_box3d_exact_pairs(ta, ta, torch.tensor([0, n, -1, 2], dtype=torch.int32, device=dev), torch.tensor([0, 0, 0, 99], dtype=torch.int32, device=dev))[1]
    assert out.tolist()[1:] == [0.0, 0.0, 0.0] and abs(float(out[0]) - 1.0) <= IOU_TOL


def test_hand_placed_emulated(emu_lib, monkeypatch):
    print("H: |hip - closed form| %.2e" % _run_hand("cpu", monkeypatch))


@pytest.mark.gpu
def test_hand_placed_gpu(hip_lib, monkeypatch):
    print("H: |hip - closed form| %.2e" % _run_hand("cuda", monkeypatch))


@pytest.mark.parametrize("name", ("Y", "T", "G"))
def test_random_sets_emulated(emu_lib, oracle_lib, monkeypatch, name):
    _run_set("cpu", name, monkeypatch, oracle_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("Y", "T", "G"))
def test_random_sets_gpu(hip_lib, oracle_lib, monkeypatch, name):
    _run_set("cuda", name, monkeypatch, oracle_lib)


def test_matrix_and_pairs_emulated(emu_lib, monkeypatch):
    _run_matrix("cpu", monkeypatch)


@pytest.mark.gpu
def test_matrix_and_pairs_gpu(hip_lib, monkeypatch):
    _run_matrix("cuda", monkeypatch)


def _argument_errors(L, dev):
    from omni3d_amd import lib
    from omni3d_amd.kernels import iou3d
    b = torch.from_numpy(boxgen.random_boxes(np.random.default_rng(0), 6)).to(dev)
    fit = iou3d.cuboid_fit(b)
    i = torch.arange(6, dtype=torch.int32, device=dev)
    for bad in (b[:, :7], b.double(), b.view(6, 24), b.transpose(1, 2).contiguous(), b[::2], b.numpy() if dev == "cpu" else None):
        with pytest.raises(ValueError):
            iou3d.cuboid_fit(bad)
    for kw in (dict(eps_dim=-1.0), dict(eps_dim=np.nan), dict(fit_tol=-1.0), dict(fit_tol=np.nan), dict(fit_tol=np.inf),
               dict(counts=torch.zeros(1, device=dev)), dict(counts=torch.zeros(2, dtype=torch.int32, device=dev))):
        with pytest.raises(ValueError):
            iou3d.cuboid_fit(b, **kw)
    for bad in ((fit[:3], fit, i, i), ((fit[0][:, :2], *fit[1:]), fit, i, i), ((fit[0].float(), *fit[1:]), fit, i, i),
                ((*fit[:3], fit[3].long()), fit, i, i), (fit, (fit[0], fit[1].view(6, 9), fit[2], fit[3]), i, i), (fit, (*fit[:2], fit[2][:5], fit[3]), i, i),
                (fit, fit, i[:5], i), (fit, fit, i.float(), i), (fit, fit, i.view(2, 3), i.view(2, 3))):
        with pytest.raises(ValueError):
            iou3d.iou_fitted_pairs(*bad)
    for bad in ((b.double(), b, i, i), (b, b[:, :7], i, i), (b, b, i[:5], i)):
        with pytest.raises(ValueError):
            iou3d.iou_box3d_exact_pairs(*bad)
    with pytest.raises(ValueError):
        iou3d.iou_box3d_exact(b, b.double())
    # the C entry points: the error status before anything touches the device, the outputs keep their poison
    outs = [torch.full(s, POISON, dtype=d, device=dev) for s, d in (((6, 3), torch.float64), ((6, 3, 3), torch.float64), ((6, 3), torch.float64), ((6,), torch.int32))]
    vol, iou = [torch.full((6,), POISON, dtype=torch.float32, device=dev) for _ in range(2)]
    P = lambda t: t.data_ptr()      # noqa: E731
    st = lib.stream_of(b)
    fitf, pairs = L._fn["omni_cuboid_fit"], L._fn["omni_iou3d_exact_pairs"]
    assert fitf(P(b), -1, EPS_DIM, FIT_TOL, *map(P, outs), None, st) == 1
    assert fitf(P(b), 6, -1.0, FIT_TOL, *map(P, outs), None, st) == 1
    assert fitf(P(b), 6, EPS_DIM, float("nan"), *map(P, outs), None, st) == 1
    assert fitf(None, 6, EPS_DIM, FIT_TOL, *map(P, outs), None, st) == 1
    assert fitf(P(b), 6, EPS_DIM, FIT_TOL, P(outs[0]), None, P(outs[2]), P(outs[3]), None, st) == 1
    assert fitf(None, 0, EPS_DIM, FIT_TOL, None, None, None, None, None, st) == 0
    assert pairs(*map(P, fit), 6, *map(P, fit), 6, P(i), P(i), -1, P(vol), P(iou), st) == 1
    assert pairs(*map(P, fit), -6, *map(P, fit), 6, P(i), P(i), 6, P(vol), P(iou), st) == 1
    assert pairs(*map(P, fit), 6, *map(P, fit), 6, None, P(i), 6, P(vol), P(iou), st) == 1
    assert pairs(*map(P, fit), 6, None, None, None, None, 6, P(i), P(i), 6, P(vol), P(iou), st) == 1
    assert pairs(*map(P, fit), 6, *map(P, fit), 6, P(i), P(i), 6, P(vol), None, st) == 1
    assert pairs(None, None, None, None, 0, None, None, None, None, 0, None, None, 0, None, None, st) == 0
    if dev == "cuda":
        torch.cuda.synchronize()
    assert all(bool((o == POISON).all()) for o in outs + [vol, iou])


def test_argument_errors_emulated(emu_lib):
    _argument_errors(emu_lib, "cpu")


@pytest.mark.gpu
def test_argument_errors_gpu(hip_lib):
    _argument_errors(hip_lib, "cuda")
