"""csrc/tp_errors.hip (`kernels.tperr`: omni_pair_errors, omni_eval_tp_errors) against tests/exact_tp_errors.py, the float64 form of
the definitions.  Every body runs under the host emulator and, marked `gpu`, on the device; outputs are poisoned before each launch.

Bounds.
  PAIR_TOL 1e-9 on every finite entry of the pair errors: both sides read the same float32 corners and work in double; double rounding
    1.1e-16 x coordinate magnitude 1e2 / smallest dimension 1e-1 x a few dozen operations is about 1e-12; 1e-9 leaves three orders and
    is still far below the 6e-6 granularity of float32 inputs at 100 m.
  AGG_TOL 2e-9 on the aggregated metrics: the pair bound plus the reordering of at most 130 non-negative double terms (1e-14).
  Closed forms: the REFERENCE is held to 1e-12 on the unrounded float64 corners (it takes any float type), the kernel to the float32
    rounding of the corners it is given: a coordinate of magnitude M is off by <= 2^-24 M, a centre (a mean) by the same, a mean edge
    by 2 x that per component, an axis direction by 2 sqrt(3) 2^-24 M / dim, two boxes and the Gram-Schmidt step double it twice:
    F32_TOL = 16 x 2^-24 x M / min(1, smallest dimension) for the boxes of each case (9.6e-7 x M / dim).

Largest |kernel - float64| (trans | scale | orient of the random pairs; the aggregated metrics), printed by every run under `-s`:
    host emulator   1.5e-13 | 0 | 4.4e-16;  6.2e-15
    MI355X          1.5e-13 | 0 | 4.4e-16;  6.2e-15
"""
import functools
import math

import numpy as np
import pytest
import torch

import exact_tp_errors as X
from omni3d_amd import boxgen

PAIR_TOL, AGG_TOL = 1e-9, 2e-9
POISON = -77.0
N_PAIRS = 2000                      # 31 workgroups and a tail of 16
UP = (0.0, -1.0, 0.0)
UP_GENERIC = (0.31, -0.87, 0.42)


def _axis_angle(axis, theta):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(theta) * K + (1 - math.cos(theta)) * (K @ K)


def _corners64(c, d, R):
    return (boxgen.UNIT * np.asarray(d, np.float64)) @ np.asarray(R, np.float64).T + np.asarray(c, np.float64)


@functools.lru_cache(maxsize=None)
def _random_pairs():
    """2 000 pairs: centres within 100 m, dimensions 0.1 .. 5, generic rotations, 1 % pairs of identical boxes; the float64 reference
    without and with two up vectors, computed once and never written to"""
    rng = np.random.default_rng(21)
    n = N_PAIRS
    c1, c2 = rng.uniform(-100, 100, (n, 3)) / math.sqrt(3), rng.uniform(-100, 100, (n, 3)) / math.sqrt(3)
    near = rng.uniform(size=n) < 0.5                               # half of the pairs are a candidate match: a few metres apart
    c2[near] = c1[near] + rng.normal(scale=1.0, size=(int(near.sum()), 3))
    d1, d2 = rng.uniform(0.1, 5, (n, 3)), rng.uniform(0.1, 5, (n, 3))
    b1, b2 = boxgen.corners(c1, d1, boxgen.rand_rot(rng, n)), boxgen.corners(c2, d2, boxgen.rand_rot(rng, n))
    same = rng.uniform(size=n) < 0.01
    b2[same] = b1[same]
    idx = np.arange(n, dtype=np.int32)
    out = dict(b1=b1, b2=b2, same=same, idx=idx)
    for name, up in (("none", None), ("up", UP), ("generic", UP_GENERIC)):
        out[name] = X.pair_errors(b1, b2, idx, idx, up)
    for v in out.values():
        v.setflags(write=False)
    return out


def test_reference_alone_meets_the_conditions():
    """no kernel: the random set has what the test is about, and the reference agrees with closed forms on unrounded corners"""
    s = _random_pairs()
    assert s["same"].sum() >= 10 and np.isfinite(s["none"]).all() and (np.abs(s["none"][s["same"]]) <= PAIR_TOL).all()
    assert np.abs(s["b1"]).max() <= 100 + 5 and (s["none"][:, 0] < 4).sum() > 400 and (s["none"][:, 0] > 50).sum() > 400
    assert (s["up"][:, 0] <= s["none"][:, 0] + 1e-12).all() and 0 <= s["none"][:, 1].min() and s["none"][:, 1].max() < 1
    assert 0 <= s["none"][:, 2].min() and s["none"][:, 2].max() <= math.pi
    for a, b, want, up in _closed_forms():
        got = X.errors(X.fit(a), X.fit(b), up)
        assert np.abs(np.array(got) - np.array(want)).max() <= 1e-12, (got, want)


def _closed_forms():
    """(detection corners, ground-truth corners, (trans, scale, orient), up) in float64, unrounded"""
    rng = np.random.default_rng(4)
    R = boxgen.rand_rot(rng, 1)[0]
    d = np.array([1.0, 0.9, 0.8])
    base = _corners64((0, 0, 0), d, R)
    cases = [(base + np.array([0.3, 7.0, 0.4]), base, (math.sqrt(0.25 + 49.0), 0.0, 0.0), None),
             (base + np.array([0.3, 7.0, 0.4]), base, (0.5, 0.0, 0.0), UP),
             (base, base, (0.0, 0.0, 0.0), None)]
    for f in (0.5, 0.8, 1.25, 3.0):
        cases.append((_corners64((0, 0, 0), f * d, R), base, (0.0, 1.0 - min(f, 1 / f) ** 3, 0.0), None))
    for theta in (0.0, 1e-6, 1.0, math.pi - 1e-6):
        axis = rng.normal(size=3)
        cases.append((_corners64((0, 0, 0), d, _axis_angle(axis, theta) @ R), base, (0.0, 0.0, theta), None))
    return cases


def _poison(monkeypatch):
    from omni3d_amd.kernels import tperr
    monkeypatch.setattr(tperr, "_empty", lambda shape, dtype, like: torch.full(shape, POISON, dtype=dtype, device=like.device))
    return tperr


def _bits(t):
    return t.cpu().contiguous().view(torch.int64)


def _run_random(dev, monkeypatch):
    from omni3d_amd.kernels import iou3d
    tperr = _poison(monkeypatch)
    s = _random_pairs()
    b1, b2 = torch.from_numpy(np.array(s["b1"])).to(dev), torch.from_numpy(np.array(s["b2"])).to(dev)
    idx = torch.from_numpy(np.array(s["idx"])).to(dev)
    f1, f2 = iou3d.cuboid_fit(b1), iou3d.cuboid_fit(b2)
    assert bool(f1[3].all()) and bool(f2[3].all())
    for name, up in (("none", None), ("up", UP), ("generic", UP_GENERIC)):
        got = tperr.pair_errors(f1, f2, idx, idx, up)
        assert got.shape == (N_PAIRS, 3) and got.dtype == torch.float64
        assert torch.equal(_bits(got), _bits(tperr.pair_errors(f1, f2, idx, idx, up)))           # two launches are bit-identical
        g = got.cpu().numpy()
        assert np.isfinite(g).all()
        worst = np.abs(g - s[name]).max(axis=0)
        print("%s: |hip - fp64| trans %.2e scale %.2e orient %.2e over %d pairs" % (name, *worst, N_PAIRS))
        assert worst.max() <= PAIR_TOL, worst
    for P in (1, 63, 64, 65):                                                                    # one thread, the wave boundary
        g = tperr.pair_errors(f1, f2, idx[:P].long(), idx[:P], None).cpu().numpy()
        assert g.shape == (P, 3) and np.abs(g - s["none"][:P]).max() <= PAIR_TOL
    none = torch.zeros(0, dtype=torch.int32, device=dev)
    assert tperr.pair_errors(f1, f2, none, none).shape == (0, 3)
    m = tperr.box3d_errors(b1[:5], b2[:3], UP).cpu().numpy()
    assert m.shape == (5, 3, 3)
    assert np.abs(m - X.pair_errors(s["b1"][:5], s["b2"][:3], np.repeat(np.arange(5), 3), np.tile(np.arange(3), 5), UP).reshape(5, 3, 3)).max() <= PAIR_TOL
    for n, k in ((0, 3), (3, 0)):
        assert tperr.box3d_errors(b1[:n], b2[:k]).shape == (n, k, 3)


def test_random_pairs_emulated(emu_lib, monkeypatch):
    _run_random("cpu", monkeypatch)


@pytest.mark.gpu
def test_random_pairs_gpu(hip_lib, monkeypatch):
    _run_random("cuda", monkeypatch)


def _run_closed_forms(dev, monkeypatch):
    tperr = _poison(monkeypatch)
    for k, (a, b, want, up) in enumerate(_closed_forms()):
        a32, b32 = a.astype(np.float32), b.astype(np.float32)
        got = tperr.box3d_errors(torch.from_numpy(a32[None]).to(dev), torch.from_numpy(b32[None]).to(dev), up).cpu().numpy()[0, 0]
        tol = 16 * 2.0 ** -24 * max(np.abs(a32).max(), np.abs(b32).max()) / min(1.0, X.fit(a)[2].min(), X.fit(b)[2].min())
        assert np.abs(got - np.array(want)).max() <= tol, (k, got, want, tol)
        ref = X.errors(X.fit(a32), X.fit(b32), up)                                               # the same float32 corners: the tight bound
        assert np.abs(got - np.array(ref)).max() <= PAIR_TOL, (k, got, ref)
    # identical boxes: (0, 0, 0) to 1e-9, wherever they are
    s = _random_pairs()
    t = torch.from_numpy(np.array(s["b1"][:40])).to(dev)
    e = tperr.box3d_errors(t, t, None).cpu().numpy()
    assert np.abs(e[np.arange(40), np.arange(40)]).max() <= 1e-9
    # the same solid with its corners listed from the opposite side (x and y axes reversed): a turn by pi, nothing else
    flipped = t[:, [2, 3, 0, 1, 6, 7, 4, 5]].contiguous()
    e = tperr.box3d_errors(flipped, t, None).cpu().numpy()[np.arange(40), np.arange(40)]
    assert np.abs(e - np.array([0.0, 0.0, math.pi])).max() <= 1e-9


def test_closed_forms_emulated(emu_lib, monkeypatch):
    _run_closed_forms("cpu", monkeypatch)


@pytest.mark.gpu
def test_closed_forms_gpu(hip_lib, monkeypatch):
    _run_closed_forms("cuda", monkeypatch)


def _run_invalid(dev, monkeypatch):
    from omni3d_amd.kernels import iou3d
    tperr = _poison(monkeypatch)
    rng = np.random.default_rng(8)
    boxes = boxgen.random_boxes(rng, 6)
    boxes[1, 5, 1] = np.nan                                                                      # a NaN vertex
    boxes[3] = boxgen.corners(np.array([[1.0, 0.5, 9.0]]), np.array([[2.0, 0.0, 1.0]]), boxgen.rand_rot(rng, 1))[0]      # a zero dimension
    t = torch.from_numpy(boxes).to(dev)
    fit = iou3d.cuboid_fit(t)
    assert fit[3].tolist() == [1, 0, 1, 0, 1, 1] and [X.fit(b) is None for b in boxes] == [False, True, False, True, False, False]
    i1 = torch.tensor([0, 1, 2, 3, 4, 6, -1, 5, 0], dtype=torch.int32, device=dev)
    i2 = torch.tensor([2, 2, 1, 0, 3, 0, 0, 99, 5], dtype=torch.int32, device=dev)
    got = tperr.pair_errors(fit, fit, i1, i2).cpu().numpy()
    want = X.pair_errors(boxes, boxes, i1.tolist(), i2.tolist())
    bad = np.array([0, 1, 1, 1, 1, 1, 1, 1, 0], bool)
    assert np.isposinf(got[bad, 0]).all() and np.isnan(got[bad, 1:]).all()
    assert np.isposinf(want[bad, 0]).all() and np.isnan(want[bad, 1:]).all()
    assert np.isfinite(got[~bad]).all() and np.abs(got[~bad] - want[~bad]).max() <= PAIR_TOL                # nothing else changes
    m = tperr.box3d_errors(t, t).cpu().numpy()
    inv = np.array([0, 1, 0, 1, 0, 0], bool)
    assert np.isposinf(m[inv, :, 0]).all() and np.isposinf(m[:, inv, 0]).all() and np.isfinite(m[~inv][:, ~inv]).all()


def test_invalid_boxes_emulated(emu_lib, monkeypatch):
    _run_invalid("cpu", monkeypatch)


@pytest.mark.gpu
def test_invalid_boxes_gpu(hip_lib, monkeypatch):
    _run_invalid("cuda", monkeypatch)


# ---- the aggregation kernel on hand-made match tables --------------------------------------------------------------------------------
LISTS = (0, 1, 63, 64, 65, 130, 0, 12, 40)         # detections per category; 6: no evaluated image, 7: recall stays low, 8: all ignored
NPIG = (0, 1, 10, 37)                             # one per "depth range"; 10 puts c / npig exactly on recall thresholds
REC_THRS = np.linspace(0.0, 1.0, 101)


@functools.lru_cache(maxsize=None)
def _tables():
    rng = np.random.default_rng(77)
    K, A, sumD, P = len(LISTS), len(NPIG), sum(LISTS), 900
    perm = rng.permutation(sumD)                                   # where the detections of the lists live
    order = perm.astype(np.int32)
    cat_off = np.concatenate([[0], np.cumsum(LISTS)]).astype(np.int32)
    err = np.stack([rng.uniform(0, 2, P), rng.uniform(0, 1, P), rng.uniform(0, math.pi, P)], 1)
    pair_row = rng.integers(0, P - 4, sumD).astype(np.int64)
    dt_match = np.full((A, sumD), -1, np.int32)
    dt_ignore = np.zeros((A, sumD), np.uint8)
    for k, n in enumerate(LISTS):
        for a, npig in enumerate(NPIG):
            tp_left = 3 if k == 7 else max(npig, 1)
            for s in range(cat_off[k], cat_off[k + 1]):
                d = order[s]
                kind = rng.uniform()
                if k == 8:
                    dt_ignore[a, d], dt_match[a, d] = 1, (int(rng.integers(0, 4)) if kind < 0.5 else -1)
                elif kind < 0.45 and tp_left > 0:
                    dt_match[a, d], tp_left = int(rng.integers(0, 4)), tp_left - 1
                elif kind < 0.6:
                    dt_ignore[a, d], dt_match[a, d] = 1, (int(rng.integers(0, 4)) if kind < 0.52 else -1)      # ignored, matched or not
    npig = np.tile(np.array(NPIG, np.int32), (K, 1))
    has_e = np.ones(K, np.int32)
    has_e[6] = 0
    out = dict(order=order, cat_off=cat_off, dt_match=dt_match, dt_ignore=dt_ignore, pair_row=pair_row, err=err, npig=npig, has_e=has_e)
    for v in out.values():
        v.setflags(write=False)
    return out


def _aggregate_reference(t, min_recall):
    K, A = len(LISTS), len(NPIG)
    want, count = -np.ones((K, A, 3)), np.zeros((K, A), np.int64)
    for k in range(K):
        for a in range(A):
            if not t["has_e"][k] or t["npig"][k, a] == 0:
                continue
            ds = [d for d in t["order"][t["cat_off"][k]:t["cat_off"][k + 1]] if not t["dt_ignore"][a, d]]
            tps = [bool(t["dt_match"][a, d] >= 0) for d in ds]
            errs = [t["err"][t["pair_row"][d] + t["dt_match"][a, d]] for d in ds if t["dt_match"][a, d] >= 0]
            want[k, a], count[k, a] = X.tp_aggregate(tps, errs, int(t["npig"][k, a]), REC_THRS, min_recall)
    return want, count


def test_aggregation_tables_have_the_cases():
    """no kernel: the hand-made tables hold what the docstrings claim"""
    t = _tables()
    want, count = _aggregate_reference(t, 0.1)
    assert (want[6] == -1).all() and (want[:, 0] == -1).all() and (count[:, 0] == 0).all()       # no evaluated image; npig == 0
    assert (want[0, 1:] == 1.0).all() and (want[8, 1:] == 1.0).all() and (count[8] == 0).all()   # an empty list, an all-ignored list
    assert count[7, 3] == 3 and (want[7, 3] == 1.0).all() and (want[7, 2] != 1.0).all()          # 3 / 37 < minRecall, 3 / 10 is not
    assert count[5, 3] == 37 and count[5, 2] == 10 and count[3, 2] == 10                           # recall reaches 1: c / 10 on thresholds
    for k in (2, 3, 4, 5):                                                                         # ignored detections between true positives
        flags = [(bool(t["dt_ignore"][3, d]), bool(t["dt_match"][3, d] >= 0)) for d in t["order"][t["cat_off"][k]:t["cat_off"][k + 1]]]
        first, last = [i for i, f in enumerate(flags) if f == (False, True)][0], [i for i, f in enumerate(flags) if f == (False, True)][-1]
        assert any(f[0] for f in flags[first:last])
    assert ((want > -1) & (want != 1.0)).sum() >= 3 * 12


def _run_aggregation(dev, monkeypatch):
    from omni3d_amd.kernels import tperr
    t = _tables()
    dv = {k: torch.from_numpy(np.array(v)).to(dev) for k, v in t.items()}
    thr = torch.from_numpy(REC_THRS).to(dev)
    for min_recall in (0.1, 0.0, 0.35):
        want, count = _aggregate_reference(t, min_recall)
        args = (dv["order"], dv["cat_off"], dv["dt_match"], dv["dt_ignore"], dv["pair_row"], dv["err"], dv["npig"], dv["has_e"], thr, min_recall)
        got, cnt = tperr.tp_errors(*args)
        again, cnt2 = tperr.tp_errors(*args)
        assert got.shape == (len(LISTS), len(NPIG), 3) and got.dtype == torch.float64 and cnt.dtype == torch.int32
        assert torch.equal(_bits(got), _bits(again)) and torch.equal(cnt.cpu(), cnt2.cpu())      # two calls: identical bits
        assert np.array_equal(cnt.cpu().numpy(), count)
        g = got.cpu().numpy()
        assert np.array_equal(g == -1, want == -1) and np.array_equal(g == 1.0, want == 1.0)
        worst = float(np.abs(g - want).max())
        print("min_recall %.2f: |hip - fp64| %.2e" % (min_recall, worst))
        assert worst <= AGG_TOL, worst
    # no category: nothing is launched
    e, c = tperr.tp_errors(dv["order"][:0], dv["cat_off"][:1], dv["dt_match"][:, :0].contiguous(), dv["dt_ignore"][:, :0].contiguous(),
                           dv["pair_row"][:0], dv["err"], dv["npig"][:0], dv["has_e"][:0], thr)
    assert e.shape == (0, len(NPIG), 3) and c.shape == (0, len(NPIG))


def test_aggregation_emulated(emu_lib, monkeypatch):
    _run_aggregation("cpu", monkeypatch)


@pytest.mark.gpu
def test_aggregation_gpu(hip_lib, monkeypatch):
    _run_aggregation("cuda", monkeypatch)


def _argument_errors(L, dev):
    from omni3d_amd import lib
    from omni3d_amd.kernels import iou3d, tperr
    b = torch.from_numpy(boxgen.random_boxes(np.random.default_rng(0), 6)).to(dev)
    fit = iou3d.cuboid_fit(b)
    i = torch.arange(6, dtype=torch.int32, device=dev)
    for bad in ((fit[:3], fit, i, i), ((fit[0].float(), *fit[1:]), fit, i, i), (fit, (fit[0], fit[1], fit[2], fit[3].long()), i, i),
                (fit, (fit[0][:5], *fit[1:]), i, i), (fit, fit, i[:5], i), (fit, fit, i.float(), i), (fit, fit, i.view(2, 3), i.view(2, 3)),
                (fit, fit, i, i, (0.0, 0.0, 0.0)), (fit, fit, i, i, (0.0, np.nan, 1.0)), (fit, fit, i, i, (1.0, 0.0))):
        with pytest.raises(ValueError):
            tperr.pair_errors(*bad)
    t = {k: torch.from_numpy(np.array(v)).to(dev) for k, v in _tables().items()}
    thr = torch.from_numpy(REC_THRS).to(dev)
    good = dict(order=t["order"], cat_off=t["cat_off"], dt_match=t["dt_match"], dt_ignore=t["dt_ignore"], pair_row=t["pair_row"], err=t["err"],
                npig=t["npig"], has_e=t["has_e"], rec_thrs=thr, min_recall=0.1)
    for key, value in (("order", t["order"].long()), ("cat_off", t["cat_off"][:-1]), ("dt_match", t["dt_match"][:, :-1].contiguous()),
                       ("dt_ignore", t["dt_ignore"].int()), ("pair_row", t["pair_row"].int()), ("err", t["err"].float()),
                       ("err", t["err"][:, :2].contiguous()), ("npig", t["npig"][:, :3].contiguous()), ("has_e", t["has_e"][:-1]),
                       ("rec_thrs", thr.float()), ("rec_thrs", thr[:0]), ("min_recall", -0.1), ("min_recall", float("nan")),
                       ("dt_match", t["dt_match"].t().contiguous().t()), ("cat_off", torch.flip(t["cat_off"], [0]))):
        with pytest.raises(ValueError):
            tperr.tp_errors(**{**good, key: value})
    # the C entry points: the error status before anything touches the device, the outputs keep their poison
    err = torch.full((6, 3), POISON, dtype=torch.float64, device=dev)
    tpe = torch.full((len(LISTS), len(NPIG), 3), POISON, dtype=torch.float64, device=dev)
    tpc = torch.full((len(LISTS), len(NPIG)), int(POISON), dtype=torch.int32, device=dev)
    P = lambda x: x.data_ptr()      # noqa: E731
    st = lib.stream_of(b)
    pairs, agg = L._fn["omni_pair_errors"], L._fn["omni_eval_tp_errors"]
    f = [P(x) for x in fit]
    assert pairs(*f, 6, *f, 6, P(i), P(i), -1, 0, 0, 0, P(err), st) == 1
    assert pairs(*f, -6, *f, 6, P(i), P(i), 6, 0, 0, 0, P(err), st) == 1
    assert pairs(*f, 6, *f, 6, None, P(i), 6, 0, 0, 0, P(err), st) == 1
    assert pairs(*f, 6, None, None, None, None, 6, P(i), P(i), 6, 0, 0, 0, P(err), st) == 1
    assert pairs(*f, 6, *f, 6, P(i), P(i), 6, 0, 0, 0, None, st) == 1
    assert pairs(*f, 6, *f, 6, P(i), P(i), 6, 0, 2.0, 0, P(err), st) == 1                         # no unit vector
    assert pairs(*f, 6, *f, 6, P(i), P(i), 6, float("nan"), 0, 0, P(err), st) == 1
    assert pairs(None, None, None, None, 0, None, None, None, None, 0, None, None, 0, 0, 0, 0, None, st) == 0
    K, A, R, sumD, NP = len(LISTS), len(NPIG), len(REC_THRS), sum(LISTS), t["err"].shape[0]
    a = [P(t[k]) for k in ("order", "cat_off", "dt_match", "dt_ignore", "pair_row", "err")]
    tail = [P(t["npig"]), P(t["has_e"]), P(thr)]
    assert agg(*a, NP, *tail, 0.1, -1, A, R, sumD, P(tpe), P(tpc), st) == 1
    assert agg(*a, NP, *tail, 0.1, K, 0, R, sumD, P(tpe), P(tpc), st) == 1
    assert agg(*a, NP, *tail, 0.1, K, A, 0, sumD, P(tpe), P(tpc), st) == 1
    assert agg(*a, NP, *tail, 0.1, K, A, R, -1, P(tpe), P(tpc), st) == 1
    assert agg(*a, -1, *tail, 0.1, K, A, R, sumD, P(tpe), P(tpc), st) == 1
    assert agg(*a, NP, *tail, 1.5, K, A, R, sumD, P(tpe), P(tpc), st) == 1
    assert agg(*a, NP, *tail, float("nan"), K, A, R, sumD, P(tpe), P(tpc), st) == 1
    assert agg(*a, NP, *tail, 0.1, K, A, R, sumD, None, P(tpc), st) == 1
    assert agg(None, *a[1:], NP, *tail, 0.1, K, A, R, sumD, P(tpe), P(tpc), st) == 1
    assert agg(*a[:5], None, NP, *tail, 0.1, K, A, R, sumD, P(tpe), P(tpc), st) == 1
    assert agg(*a, NP, None, *tail[1:], 0.1, K, A, R, sumD, P(tpe), P(tpc), st) == 1
    assert agg(None, None, None, None, None, None, 0, None, None, None, 0.1, 0, A, R, 0, None, None, st) == 0
    if dev == "cuda":
        torch.cuda.synchronize()
    assert bool((err == POISON).all()) and bool((tpe == POISON).all()) and bool((tpc == int(POISON)).all())


def test_argument_errors_emulated(emu_lib):
    _argument_errors(emu_lib, "cpu")


@pytest.mark.gpu
def test_argument_errors_gpu(hip_lib):
    _argument_errors(hip_lib, "cuda")
