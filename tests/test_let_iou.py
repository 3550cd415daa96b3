"""csrc/let_iou.hip (`kernels.let`: omni_let_pairs, omni_eval_accumulate_let) against tests/exact_let.py, the float64 form of the
definitions.  Every body runs under the host emulator and, marked `gpu`, on the device; outputs are poisoned before each launch.

Bounds.
  IOU_TOL 1e-5 absolute on let_iou: the project's IoU3D bound (`IOU_TOL` of tests/test_iou3d_exact.py).
  PAIR_TOL 1e-9 on aff and lon: both sides read the same float32 corners and work in double (the reasoning of `PAIR_TOL` in
    tests/test_tp_errors.py: 1.1e-16 x 40 m / a tolerance of 0.5 m x a few dozen operations is about 1e-13).
  AGG_TOL 2e-9 on precision_l, tp_affinity, tp_lon: the pair bound plus the reordering of at most about 130 terms (1e-14).
  Gated pairs are exact: (0, 0, NaN).
  On the gate: a pair with | |lon| / T - 1 | < 1e-6 may be excluded (let_iou jumps there), at most 1 % of a set; set M has none.
  Closed forms (set H) hold the kernel to the float32 rounding of the corners it is given, F32_TOL = 16 x 2^-24 x M / min(1, smallest
    dimension) of tests/test_tp_errors.py on lon; aff = 1 - |lon| / T moves by at most 2 F32_TOL / T (lon and T both move); an IoU
    of 1 loses at most the relative displacement F32_TOL / dimension on each of the three axes, for each of the two boxes: 6 F32_TOL /
    smallest dimension.

Largest |kernel - float64| (let_iou | aff | lon of set M; precision_l | tp_affinity | tp_lon of the synthetic table), printed by
every run under `-s`:
    host emulator   0 | 3.3e-16 | 8.9e-16;  1.1e-16 | 1.1e-16 | 5.6e-17
    MI355X          0 | 3.3e-16 | 8.9e-16;  1.1e-16 | 1.1e-16 | 5.6e-17
"""
import functools
import math

import numpy as np
import pytest
import torch

import exact_let as X
from exact_tp_errors import fit as xfit
from omni3d_amd import boxgen

IOU_TOL, PAIR_TOL, AGG_TOL = 1e-5, 1e-9, 2e-9
GATE_BAND, GATE_CAP = 1e-6, 0.01
POISON = -77.0
N_PAIRS = 400                       # six workgroups and a tail of 16
SEED_M = 5
THRS = (0.05, 0.15, 0.25, 0.5)


def _corners64(c, d, R):
    return (boxgen.UNIT * np.asarray(d, np.float64)) @ np.asarray(R, np.float64).T + np.asarray(c, np.float64)


def _nearest_rotation(m):
    u, _, vt = np.linalg.svd(m)
    r = u @ vt
    if np.linalg.det(r) < 0:
        r = u @ np.diag([1.0, 1.0, -1.0]) @ vt
    return r


def make_set(rng, n):
    """ground truths like boxgen.omni3d_like_pairs (centres U[-5,5] x U[-2,2] x U[2,40], dimensions U[0.2,5], random rotations);
    detection = its ground truth moved along its line of sight by N(0, 0.08) x range, jittered laterally by N(0, 0.1) x dimensions
    (in the box frame), dimensions x U[0.8, 1.25], rotation blended 10 % towards a random one -> (dt (n,8,3), gt (n,8,3)) float32"""
    cg = np.stack([rng.uniform(-5, 5, n), rng.uniform(-2, 2, n), rng.uniform(2, 40, n)], 1)
    dg = rng.uniform(0.2, 5, (n, 3))
    Rg = boxgen.rand_rot(rng, n)
    rngs = np.linalg.norm(cg, axis=1, keepdims=True)
    slide = rng.normal(0, 0.08, (n, 1)) * rngs
    jitter = np.einsum("nij,nj->ni", Rg, rng.normal(0, 0.1, (n, 3)) * dg)
    cd = cg + slide * cg / rngs + jitter
    dd = dg * rng.uniform(0.8, 1.25, (n, 3))
    Rr = boxgen.rand_rot(rng, n)
    Rd = np.stack([_nearest_rotation(0.9 * Rg[i] + 0.1 * Rr[i]) for i in range(n)])
    return boxgen.corners(cd, dd, Rd), boxgen.corners(cg, dg, Rg)


def on_gate(aff_ref, lon_ref, boxes_gt, tol_frac=0.1, tol_min=0.5):
    """pairs within GATE_BAND of the gate, by the reference alone"""
    out = np.zeros(len(lon_ref), bool)
    for p, b in enumerate(boxes_gt):
        f = xfit(b)
        if f is not None and np.isfinite(lon_ref[p]):
            T = max(tol_frac * float(np.linalg.norm(f[0])), tol_min)
            out[p] = abs(abs(lon_ref[p]) / T - 1.0) < GATE_BAND
    return out


@functools.lru_cache(maxsize=None)
def _set_m():
    """set M and its float64 reference, computed once and never written to"""
    dt, gt = make_set(np.random.default_rng(SEED_M), N_PAIRS)
    idx = np.arange(N_PAIRS, dtype=np.int32)
    iou, aff, lon = X.let_pairs(dt, gt, idx, idx)
    out = dict(dt=dt, gt=gt, idx=idx, iou=iou, aff=aff, lon=lon, gate=on_gate(aff, lon, gt))
    for v in out.values():
        v.setflags(write=False)
    return out


def test_reference_alone_meets_the_conditions():
    """no kernel: set M has what the test is about, and the reference agrees with the closed forms on unrounded corners"""
    s = _set_m()
    gated = s["aff"] == 0
    assert np.isfinite(s["lon"]).all() and (s["iou"][gated] == 0).all()
    plain = X.plain_iou(s["dt"], s["gt"])
    gain = s["iou"] - plain
    print("set M: %d ungated, %d gated, %d on the gate; mean LET-IoU %.3f against plain %.3f; %d gain > 0.01; IoU >= 0.5: %d against %d"
          % ((~gated).sum(), gated.sum(), s["gate"].sum(), s["iou"].mean(), plain.mean(), (gain > 0.01).sum(), (s["iou"] >= 0.5).sum(),
             (plain >= 0.5).sum()))
    assert gated.sum() >= 50 and (~gated).sum() >= 200 and (gain > 0.01).sum() >= 100
    assert s["gate"].sum() == 0
    assert min(np.abs(s["iou"][~gated] - t).min() for t in THRS) > 1e-4
    for a, b, want in _closed_forms():
        got = X.let_pair(xfit(a), xfit(b), iou=False)
        for g, w in zip(got, want):
            if w is not None and g is not None:
                assert (math.isnan(g) and math.isnan(w)) or abs(g - w) <= 1e-12, (got, want)


def _closed_forms():
    """set H: (detection corners, ground-truth corners, (let_iou or None, aff, lon)) in float64, unrounded"""
    rng = np.random.default_rng(4)
    R = boxgen.rand_rot(rng, 1)[0]
    d = np.array([1.0, 0.9, 0.8])
    cases = []
    for rng_m, slide, aff in ((20.0, 1.0, 0.5), (20.0, -1.0, 0.5), (3.0, 0.25, 0.5), (3.0, -0.25, 0.5),      # 5 % of 20 m; tol_min rules at 3 m
                              (20.0, 2.0 * (1 - 1e-3), 1e-3), (20.0, -2.0 * (1 - 1e-3), 1e-3),              # just inside T
                              (20.0, 2.0 * (1 + 1e-3), 0.0), (20.0, -2.0 * (1 + 1e-3), 0.0)):               # just outside: 0 / 0
        u = np.array([2.0, -1.0, 6.0])
        u /= np.linalg.norm(u)
        G = rng_m * u
        cases.append((_corners64(G - slide * u, d, R), _corners64(G, d, R), (1.0 if aff > 0 else 0.0, aff, slide)))
    # a purely lateral offset s: lon = -s^2 / |P|
    G = np.array([0.0, 0.0, 20.0])
    for s in (0.5, 3.0):
        P = G + np.array([s, 0.0, 0.0])
        lon = -s * s / math.sqrt(400.0 + s * s)
        cases.append((_corners64(P, d, R), _corners64(G, d, R), (None, 1.0 - abs(lon) / 2.0, lon)))
    return cases


def _poison(monkeypatch):
    from omni3d_amd.kernels import let
    monkeypatch.setattr(let, "_empty", lambda shape, dtype, like: torch.full(shape, POISON, dtype=dtype, device=like.device))
    return let


def _bits(t):
    t = t.cpu().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int64)


def _same_bits(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _run_set_m(dev, monkeypatch):
    from omni3d_amd.kernels import iou3d
    let = _poison(monkeypatch)
    s = _set_m()
    dt, gt = torch.from_numpy(np.array(s["dt"])).to(dev), torch.from_numpy(np.array(s["gt"])).to(dev)
    idx = torch.from_numpy(np.array(s["idx"])).to(dev)
    f1, f2 = iou3d.cuboid_fit(dt), iou3d.cuboid_fit(gt)
    got = let.let_pairs(f1, f2, idx, idx)
    assert [g.dtype for g in got] == [torch.float32, torch.float64, torch.float64] and all(g.shape == (N_PAIRS,) for g in got)
    assert _same_bits(got, let.let_pairs(f1, f2, idx, idx))                                       # two launches are bit-identical
    iou, aff, lon = (g.cpu().numpy().astype(np.float64) for g in got)
    assert np.isfinite(iou).all() and np.isfinite(aff).all() and (iou >= 0).all() and (iou <= 1).all() and (aff >= 0).all() and (aff <= 1).all()
    keep = ~s["gate"]
    assert (~keep).sum() <= GATE_CAP * N_PAIRS
    worst = [np.abs(iou - s["iou"])[keep].max(), np.abs(aff - s["aff"])[keep].max(), np.abs(lon - s["lon"])[keep].max()]
    print("set M: |hip - fp64| let_iou %.2e aff %.2e lon %.2e over %d pairs (%d excluded on the gate)" % (*worst, keep.sum(), (~keep).sum()))
    assert worst[0] <= IOU_TOL and worst[1] <= PAIR_TOL and worst[2] <= PAIR_TOL, worst
    gated = s["aff"] == 0
    assert (iou[gated & keep] == 0).all() and (aff[gated & keep] == 0).all()
    for P in (1, 64, 65):                                                                         # one thread, the wave boundary
        part = let.let_pairs(f1, f2, idx[:P].long(), idx[:P])
        assert _same_bits(part, [g[:P] for g in got])
    none = torch.zeros(0, dtype=torch.int32, device=dev)
    assert [g.shape for g in let.let_pairs(f1, f2, none, none)] == [(0,)] * 3
    # the full index grid
    m = let.box3d_let(dt[:5], gt[:7])
    i1, i2 = torch.arange(5, device=dev).repeat_interleave(7), torch.arange(7, device=dev).repeat(5)
    assert all(g.shape == (5, 7) for g in m) and _same_bits([g.reshape(-1) for g in m], let.let_pairs(f1, f2, i1, i2))
    assert _same_bits([g.diagonal() for g in m], [g[:5] for g in got])
    for n, k in ((0, 3), (3, 0)):
        assert [g.shape for g in let.box3d_let(dt[:n], gt[:k])] == [(n, k)] * 3
    # other tolerances: the reference without Qhull
    for tf, tm in ((0.0, 0.5), (0.05, 2.0)):
        _, aff2, lon2 = (g.cpu().numpy() for g in let.let_pairs(f1, f2, idx, idx, tf, tm))
        _, wa, wl = X.let_pairs(s["dt"], s["gt"], s["idx"], s["idx"], tf, tm, iou=False)
        assert np.abs(aff2 - wa).max() <= PAIR_TOL and np.abs(lon2 - wl).max() <= PAIR_TOL


def test_set_m_emulated(emu_lib, monkeypatch):
    _run_set_m("cpu", monkeypatch)


@pytest.mark.gpu
def test_set_m_gpu(hip_lib, monkeypatch):
    _run_set_m("cuda", monkeypatch)


def _run_closed_forms(dev, monkeypatch):
    let = _poison(monkeypatch)
    for k, (a, b, want) in enumerate(_closed_forms()):
        a32, b32 = a.astype(np.float32), b.astype(np.float32)
        iou, aff, lon = (float(g.cpu().numpy()[0, 0]) for g in let.box3d_let(torch.from_numpy(a32[None]).to(dev), torch.from_numpy(b32[None]).to(dev)))
        dmin = min(xfit(a)[2].min(), xfit(b)[2].min())
        tol = 16 * 2.0 ** -24 * max(np.abs(a32).max(), np.abs(b32).max()) / min(1.0, dmin)
        T = max(0.1 * float(np.linalg.norm(b.mean(axis=0))), 0.5)
        assert abs(lon - want[2]) <= tol, (k, lon, want, tol)
        if want[1] == 0.0:
            assert aff == 0.0 and iou == 0.0, (k, iou, aff)                                      # outside T: exactly 0 / 0
        else:
            assert abs(aff - want[1]) <= 2 * tol / T, (k, aff, want, tol)
            if want[0] is not None:
                assert abs(iou - want[0]) <= 6 * tol / dmin, (k, iou, want, tol)


def test_closed_forms_emulated(emu_lib, monkeypatch):
    _run_closed_forms("cpu", monkeypatch)


@pytest.mark.gpu
def test_closed_forms_gpu(hip_lib, monkeypatch):
    _run_closed_forms("cuda", monkeypatch)


def _run_gated(dev, monkeypatch):
    from omni3d_amd.kernels import iou3d
    let = _poison(monkeypatch)
    rng = np.random.default_rng(8)
    boxes = boxgen.random_boxes(rng, 7) + np.array([0.0, 0.0, 9.0], np.float32)
    boxes[1, 5, 1] = np.nan                                                                      # a NaN vertex
    boxes[3] = boxgen.corners(np.array([[1.0, 0.5, 9.0]]), np.array([[2.0, 0.0, 1.0]]), boxgen.rand_rot(rng, 1))[0]      # a zero dimension
    boxes[5, 2] += np.array([0.3, -0.2, 0.4], np.float32)                                        # a displaced vertex: no cuboid
    boxes[6] = boxgen.corners(np.zeros((1, 3)), np.array([[1.0, 2.0, 0.5]]), np.eye(3)[None])[0]  # centred on the sensor
    t = torch.from_numpy(boxes).to(dev)
    fit = iou3d.cuboid_fit(t)
    assert fit[3].tolist() == [1, 0, 1, 0, 1, 0, 1] and [xfit(b) is None for b in boxes] == [False, True, False, True, False, True, False]
    assert bool((fit[0][6] == 0).all())
    #                    ok ok  bad on either side     outside the set   on the sensor (as a detection only)
    i1 = torch.tensor([0, 2, 1, 0, 3, 4, 5, 2, 7, -1, 4, 0, 6, 0], dtype=torch.int32, device=dev)
    i2 = torch.tensor([2, 4, 0, 1, 2, 3, 0, 5, 0, 0, 99, -3, 0, 6], dtype=torch.int32, device=dev)
    bad = np.array([0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0], bool)
    iou, aff, lon = (g.cpu().numpy() for g in let.let_pairs(fit, fit, i1, i2))
    wi, wa, wl = X.let_pairs(boxes, boxes, i1.tolist(), i2.tolist())
    for a, b, c in ((iou, aff, lon), (wi, wa, wl)):
        assert (a[bad] == 0).all() and (b[bad] == 0).all() and np.isnan(c[bad]).all() and np.isfinite(c[~bad]).all()
    assert np.abs(iou[~bad] - wi[~bad]).max() <= IOU_TOL and np.abs(aff[~bad] - wa[~bad]).max() <= PAIR_TOL          # nothing else changes
    assert np.abs(lon[~bad] - wl[~bad]).max() <= PAIR_TOL
    m = [g.cpu().numpy() for g in let.box3d_let(t, t)]
    inv = np.array([0, 1, 0, 1, 0, 1, 0], bool)
    assert (m[0][inv] == 0).all() and (m[0][:, inv] == 0).all() and np.isnan(m[2][inv]).all() and np.isnan(m[2][:, inv]).all()
    assert np.isnan(m[2][6]).all() and np.isfinite(m[2][~inv][:-1][:, ~inv]).all() and not np.isnan(m[0]).any() and not np.isnan(m[1]).any()


def test_gated_pairs_emulated(emu_lib, monkeypatch):
    _run_gated("cpu", monkeypatch)


@pytest.mark.gpu
def test_gated_pairs_gpu(hip_lib, monkeypatch):
    _run_gated("cuda", monkeypatch)


# ---- the accumulation kernel on a synthetic table -------------------------------------------------------------------------------------
LISTS = (129, 130, 131, 40, 0)      # detections per category; 0..2 span three chunks, 3: no evaluated image, 4: no detections
NPIG = ((40, 0), (10, 37), (25, 60), (5, 5), (7, 3))       # (K, A); category 0 has no ground truth in range 1; 10 puts c / npig on thresholds
MAX_DETS = (1, 10, 100)
T_ACC = 2
REC_THRS = np.linspace(0.0, 1.0, 101)


@functools.lru_cache(maxsize=None)
def _tables():
    rng = np.random.default_rng(77)
    K, A, T, sumD, P = len(LISTS), 2, T_ACC, sum(LISTS), 900
    cat = rng.permutation(np.repeat(np.arange(K), LISTS))          # the category of every detection, in storage order
    rank, score = np.zeros(sumD, np.int32), np.zeros(sumD)
    for k in range(K):                                             # the category's detections fall into images of 5 .. 14
        mine, at = np.flatnonzero(cat == k), 0
        while at < len(mine):
            n = min(int(rng.integers(5, 15)), len(mine) - at)
            rank[mine[at:at + n]] = np.arange(n)
            score[mine[at:at + n]] = np.sort(rng.integers(0, 40, n) / 40.0)[::-1]      # a coarse grid: ties within and across images
            at += n
    order = np.lexsort((np.arange(sumD), -score, cat)).astype(np.int32)
    cat_off = np.concatenate([[0], np.cumsum(LISTS)]).astype(np.int32)
    aff = rng.uniform(0, 1, P)
    aff[rng.uniform(size=P) < 0.1] = 1.0
    aff[rng.uniform(size=P) < 0.1] = 0.0
    lon = rng.normal(0, 1, P)
    pair_row = rng.integers(0, P - 4, sumD).astype(np.int64)
    dt_match = np.full((A, T, sumD), -1, np.int32)
    dt_ignore = np.zeros((A, T, sumD), np.uint8)
    for k in range(K):
        for a in range(A):
            for t in range(T):
                tp_left = max(NPIG[k][a], 1)
                for s in range(cat_off[k], cat_off[k + 1]):
                    d, kind = order[s], rng.uniform()
                    if kind < 0.45 and tp_left > 0:
                        dt_match[a, t, d], tp_left = int(rng.integers(0, 4)), tp_left - 1
                    elif kind < 0.6:
                        dt_ignore[a, t, d], dt_match[a, t, d] = 1, (int(rng.integers(0, 4)) if kind < 0.52 else -1)
    npig = np.array(NPIG, np.int32)
    has_e = np.ones(K, np.int32)
    has_e[3] = 0
    out = dict(order=order, cat_off=cat_off, rank=rank, score=score, dt_match=dt_match, dt_ignore=dt_ignore, pair_row=pair_row, aff=aff,
               lon=lon, npig=npig, has_e=has_e, max_dets=np.array(MAX_DETS, np.int32))
    for v in out.values():
        v.setflags(write=False)
    return out


def _acc_reference(t, aff=None):
    return X.accumulate(t["order"], t["cat_off"], t["rank"], t["dt_match"], t["dt_ignore"], t["pair_row"], t["aff"] if aff is None else aff,
                        t["lon"], t["npig"], t["has_e"], REC_THRS, list(MAX_DETS))


def test_accumulation_table_has_the_cases():
    """no kernel: the synthetic table holds what the docstrings claim"""
    t = _tables()
    w = _acc_reference(t)
    assert (w["precision_l"][:, :, 3] == -1).all() and (w["precision_l"][:, :, 0, 1] == -1).all()          # has_e == 0; npig == 0
    assert (w["precision_l"][:, :, 4] == 0).all() and (w["tp_affinity"][:, 4] == -1).all()                 # no detections
    assert np.array_equal(w["precision_l"] == -1, w["precision"] == -1)
    assert (w["precision_l"] <= w["precision"] + 1e-15).all() and (w["precision_l"][w["precision"] > 0] < w["precision"][w["precision"] > 0]).any()
    assert (w["tp_affinity"][:, :3, 0] > 0).all() and (w["tp_lon"][:, :3, 0] != -1).all()
    for k in range(3):                                                                                     # ties in score inside a category
        sc = t["score"][t["order"][t["cat_off"][k]:t["cat_off"][k + 1]]]
        assert (np.diff(sc) == 0).sum() >= 20 and (np.diff(sc) <= 0).all()


def _run_accumulation(dev, monkeypatch):
    from omni3d_amd import lib
    from omni3d_amd.kernels import let
    t = _tables()
    dv = {k: torch.from_numpy(np.array(v)).to(dev) for k, v in t.items()}
    thr = torch.from_numpy(REC_THRS).to(dev)
    K, A, T, R, M, sumD = len(LISTS), 2, T_ACC, len(REC_THRS), len(MAX_DETS), sum(LISTS)
    args = lambda aff: (dv["order"], dv["cat_off"], dv["rank"], dv["dt_match"], dv["dt_ignore"], dv["pair_row"], aff, dv["lon"], dv["npig"],      # noqa: E731
                        dv["has_e"], thr, dv["max_dets"])
    # precision of the existing kernel on the same tables
    prec = torch.full((T, R, K, A, M), -1.0, dtype=torch.float64, device=dev)
    rec = torch.full((T, K, A, M), -1.0, dtype=torch.float64, device=dev)
    scr = torch.full((T, R, K, A, M), -1.0, dtype=torch.float64, device=dev)
    p = lib.ptr
    lib.get().call("omni_eval_accumulate", p(dv["order"]), p(dv["cat_off"]), p(dv["rank"]), p(dv["score"]), p(dv["dt_match"]), p(dv["dt_ignore"]),
                   p(dv["npig"]), p(dv["has_e"]), p(thr), p(dv["max_dets"]), K, A, M, T, R, sumD, p(prec), p(rec), p(scr), lib.stream_of(prec))
    prec = prec.cpu().numpy()
    want = _acc_reference(t)
    assert np.abs(prec - want["precision"]).max() <= 1e-12
    got = let.accumulate_let(*args(dv["aff"]))
    assert [g.shape for g in got] == [(T, R, K, A, M), (T, K, A, M), (T, K, A, M)] and all(g.dtype == torch.float64 for g in got)
    assert _same_bits(got, let.accumulate_let(*args(dv["aff"])))                                  # two launches: identical bits
    pl, ta, tl = (g.cpu().numpy() for g in got)
    assert np.array_equal(pl == -1, prec == -1) and np.array_equal(ta == -1, want["tp_affinity"] == -1)
    assert np.array_equal(tl == -1, want["tp_lon"] == -1)
    worst = [np.abs(pl - want["precision_l"]).max(), np.abs(ta - want["tp_affinity"]).max(), np.abs(tl - want["tp_lon"]).max()]
    print("synthetic table: |hip - fp64| precision_l %.2e tp_affinity %.2e tp_lon %.2e" % tuple(worst))
    assert max(worst) <= AGG_TOL, worst
    assert (pl <= prec + AGG_TOL).all()
    # all aff = 1: the longitudinal precision is the precision
    ones = torch.ones_like(dv["aff"])
    pl1, ta1, _ = (g.cpu().numpy() for g in let.accumulate_let(*args(ones)))
    assert np.abs(pl1 - prec).max() <= AGG_TOL and (ta1[ta1 > -1] == 1.0).all()
    # more than 64 recall thresholds are walked in batches: a second grid with 130 of them, and one with a single threshold
    for grid in (np.linspace(0.0, 1.0, 130), np.array([0.5])):
        g = let.accumulate_let(*args(dv["aff"])[:10], torch.from_numpy(grid).to(dev), dv["max_dets"])[0].cpu().numpy()
        w = X.accumulate(t["order"], t["cat_off"], t["rank"], t["dt_match"], t["dt_ignore"], t["pair_row"], t["aff"], t["lon"], t["npig"],
                         t["has_e"], grid, list(MAX_DETS))["precision_l"]
        assert np.abs(g - w).max() <= AGG_TOL
    # no category: nothing is launched
    e = let.accumulate_let(dv["order"][:0], dv["cat_off"][:1], dv["rank"][:0], dv["dt_match"][:, :, :0].contiguous(),
                           dv["dt_ignore"][:, :, :0].contiguous(), dv["pair_row"][:0], dv["aff"], dv["lon"], dv["npig"][:0], dv["has_e"][:0], thr,
                           dv["max_dets"])
    assert [g.shape for g in e] == [(T, R, 0, A, M), (T, 0, A, M), (T, 0, A, M)]


def test_accumulation_emulated(emu_lib, monkeypatch):
    _run_accumulation("cpu", monkeypatch)


@pytest.mark.gpu
def test_accumulation_gpu(hip_lib, monkeypatch):
    _run_accumulation("cuda", monkeypatch)


def _argument_errors(L, dev):
    from omni3d_amd import lib
    from omni3d_amd.kernels import iou3d, let
    b = torch.from_numpy(boxgen.random_boxes(np.random.default_rng(0), 6) + np.array([0, 0, 9], np.float32)).to(dev)
    fit = iou3d.cuboid_fit(b)
    i = torch.arange(6, dtype=torch.int32, device=dev)
    for bad in ((fit[:3], fit, i, i), ((fit[0].float(), *fit[1:]), fit, i, i), (fit, (fit[0], fit[1], fit[2], fit[3].long()), i, i),
                (fit, (fit[0][:5], *fit[1:]), i, i), (fit, fit, i[:5], i), (fit, fit, i.float(), i), (fit, fit, i.view(2, 3), i.view(2, 3)),
                (fit, fit, i, i, -0.1), (fit, fit, i, i, float("nan")), (fit, fit, i, i, float("inf")), (fit, fit, i, i, 0.1, 0.0),
                (fit, fit, i, i, 0.1, -1.0), (fit, fit, i, i, 0.1, float("nan")), (fit, fit, i, i, 0.1, float("inf")), (fit, fit, i, i, "a")):
        with pytest.raises(ValueError):
            let.let_pairs(*bad)
    for bad in ((b, b, -0.1), (b, b, 0.1, 0.0), (b[:, :7], b), (b.double(), b)):
        with pytest.raises(ValueError):
            let.box3d_let(*bad)
    t = {k: torch.from_numpy(np.array(v)).to(dev) for k, v in _tables().items()}
    thr = torch.from_numpy(REC_THRS).to(dev)
    good = dict(order=t["order"], cat_off=t["cat_off"], rank=t["rank"], dt_match=t["dt_match"], dt_ignore=t["dt_ignore"], pair_row=t["pair_row"],
                aff=t["aff"], lon=t["lon"], npig=t["npig"], has_e=t["has_e"], rec_thrs=thr, max_dets=t["max_dets"])
    let.accumulate_let(**good)
    for key, value in (("order", t["order"].long()), ("order", t["order"] + 1), ("cat_off", t["cat_off"][:-1]), ("rank", t["rank"][:-1]),
                       ("rank", t["rank"].long()), ("dt_match", t["dt_match"][:, :, :-1].contiguous()), ("dt_match", t["dt_match"][0]),
                       ("dt_ignore", t["dt_ignore"].int()), ("pair_row", t["pair_row"].int()), ("aff", t["aff"].float()),
                       ("aff", t["aff"][:-1]), ("lon", t["lon"].view(-1, 1)), ("npig", t["npig"][:, :1].contiguous()), ("has_e", t["has_e"][:-1]),
                       ("rec_thrs", thr.float()), ("rec_thrs", thr[:0]), ("max_dets", t["max_dets"].long()), ("max_dets", t["max_dets"][:0]),
                       ("dt_match", t["dt_match"].transpose(0, 1).contiguous().transpose(0, 1)), ("cat_off", torch.flip(t["cat_off"], [0]))):
        with pytest.raises(ValueError):
            let.accumulate_let(**{**good, key: value})
    # the C entry points: the error status before anything touches the device, the outputs keep their poison
    K, A, T, R, M, sumD, NP = len(LISTS), 2, T_ACC, len(REC_THRS), len(MAX_DETS), sum(LISTS), t["aff"].shape[0]
    o_iou = torch.full((6,), POISON, dtype=torch.float32, device=dev)
    o_aff, o_lon = torch.full((6,), POISON, dtype=torch.float64, device=dev), torch.full((6,), POISON, dtype=torch.float64, device=dev)
    o_pl = torch.full((T, R, K, A, M), POISON, dtype=torch.float64, device=dev)
    o_ta, o_tl = torch.full((T, K, A, M), POISON, dtype=torch.float64, device=dev), torch.full((T, K, A, M), POISON, dtype=torch.float64, device=dev)
    P = lambda x: x.data_ptr()      # noqa: E731
    st = lib.stream_of(b)
    pairs, acc = L._fn["omni_let_pairs"], L._fn["omni_eval_accumulate_let"]
    f = [P(x) for x in fit]
    out = [P(o_iou), P(o_aff), P(o_lon)]
    assert pairs(*f, 6, *f, 6, P(i), P(i), -1, 0.1, 0.5, *out, st) == 1
    assert pairs(*f, -6, *f, 6, P(i), P(i), 6, 0.1, 0.5, *out, st) == 1
    assert pairs(*f, 6, *f, 6, None, P(i), 6, 0.1, 0.5, *out, st) == 1
    assert pairs(*f, 6, None, None, None, None, 6, P(i), P(i), 6, 0.1, 0.5, *out, st) == 1
    assert pairs(*f, 6, *f, 6, P(i), P(i), 6, 0.1, 0.5, None, *out[1:], st) == 1
    assert pairs(*f, 6, *f, 6, P(i), P(i), 6, 0.1, 0.5, *out[:2], None, st) == 1
    for tf, tm in ((-0.1, 0.5), (float("nan"), 0.5), (float("inf"), 0.5), (0.1, 0.0), (0.1, -1.0), (0.1, float("nan")), (0.1, float("inf"))):
        assert pairs(*f, 6, *f, 6, P(i), P(i), 6, tf, tm, *out, st) == 1
    assert pairs(None, None, None, None, 0, None, None, None, None, 0, None, None, 0, 0.1, 0.5, None, None, None, st) == 0
    a = [P(t[k]) for k in ("order", "cat_off", "rank", "dt_match", "dt_ignore", "pair_row", "aff", "lon")]
    tail = [P(t["npig"]), P(t["has_e"]), P(thr), P(t["max_dets"])]
    res = [P(o_pl), P(o_ta), P(o_tl)]
    for sizes in ((-1, A, M, T, R, sumD), (K, 0, M, T, R, sumD), (K, A, 0, T, R, sumD), (K, A, M, 0, R, sumD), (K, A, M, T, 0, sumD),
                  (K, A, M, T, R, -1)):
        assert acc(*a, NP, *tail, *sizes, *res, st) == 1
    assert acc(*a, -1, *tail, K, A, M, T, R, sumD, *res, st) == 1
    assert acc(*a, NP, *tail, K, A, M, T, R, sumD, None, *res[1:], st) == 1
    assert acc(*a, NP, *tail, K, A, M, T, R, sumD, *res[:2], None, st) == 1
    assert acc(None, *a[1:], NP, *tail, K, A, M, T, R, sumD, *res, st) == 1
    assert acc(*a[:6], None, a[7], NP, *tail, K, A, M, T, R, sumD, *res, st) == 1
    assert acc(*a, NP, None, *tail[1:], K, A, M, T, R, sumD, *res, st) == 1
    assert acc(None, None, None, None, None, None, None, None, 0, None, None, None, None, 0, A, M, T, R, 0, None, None, None, st) == 0
    if dev == "cuda":
        torch.cuda.synchronize()
    assert all(bool((o == POISON).all()) for o in (o_iou, o_aff, o_lon, o_pl, o_ta, o_tl))


def test_argument_errors_emulated(emu_lib):
    _argument_errors(emu_lib, "cpu")


@pytest.mark.gpu
def test_argument_errors_gpu(hip_lib):
    _argument_errors(hip_lib, "cuda")
