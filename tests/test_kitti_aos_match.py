"""`match_counts_aos` / `finalize_aos` / `run_aos` (`kernels.kitti`, csrc/eval_kitti.hip) against the float64 loops of
tests/exact_kitti_aos.py, on synthetic similarity matrices in the style and the shapes of tests/test_kitti_match.py (D in {0, 1, 63, 64,
65, 130, 1024}, G in {0, 1, 40, 81}, 257 images, scores and overlaps that tie) with headings fed directly: no geometry is involved.

Bars.  `counts` are the bits of `match_counts`.  `sim_sum[s, k]` is the oracle's sum of rint(q 2^40) within tp[s, k] units: the two
`cos` implementations may round one term one unit apart.  `aos` and `aos_ap` are within 1e-9 of the oracle's float64 values: a term is
off by at most 2^-40 (half a unit of rounding, one unit of cos), the sum of at most tp of them is divided by tp + fp >= tp, and times 100
that is <= 1e-10.  Two runs give the same bits.  Every output is poisoned before its launch."""
import functools
import types

import numpy as np
import pytest
import torch

import exact_kitti as X
import exact_kitti_aos as XA
from test_kitti_match import CLS_TAB, DIFFS, _image, _problem, _slots, _sorted

TAB = {"cls_tab": CLS_TAB[:1], "diffs": DIFFS[:1], "min_ov": [[0.7]], "dc_metric": [1, 0, 1]}      # cars at Easy, M = 3: slots = metrics
AOS_METRIC = (1, 0, 0)
BIG = [(0, 1, 0), (1, 0, 1), (63, 40, 2), (64, 1, 1), (65, 81, 0), (130, 40, 3), (1024, 1, 1), (1, 1, 0), (0, 0, 0), (130, 81, 1)]
N_IMG = 257


@functools.lru_cache(maxsize=None)
def _case():
    """257 images: the sizes of BIG and small ones; headings uniform in (-pi, pi], a tenth NaN on each side, a quarter of the
    detections with the heading of a ground truth of their image, a sixth with that heading plus pi"""
    rng = np.random.default_rng(23)
    sizes = BIG + [(int(rng.integers(0, 7)), int(rng.integers(0, 5)), int(rng.integers(0, 2))) for _ in range(N_IMG - len(BIG))]
    images = []
    for D, G, R in sizes:
        # as `_random_images` of test_kitti_match.py (overlaps multiples of 1/8, scores of 1/20: ties all the time), with more cars in the
        # small images, more overlaps and more boxes of full height, so that the slots reach many thresholds
        im = _image(D, G, R, 3)
        im["sim"] = rng.choice([0.0, 0.25, 0.5, 0.625, 0.75, 0.875, 1.0], (3, D, G), p=[0.4, 0.05, 0.05, 0.1, 0.1, 0.15, 0.15]).astype(np.float32)
        im["dc"] = (rng.integers(0, 9, (D, R)) / 8.0).astype(np.float32) * (rng.uniform(size=(D, R)) < 0.3)
        car = 0.7 if D < 63 else 0.15                        # the crowded images hold mostly other things: fewer false positives
        im["dt_code"] = rng.choice([0, 5, 1, 3, 7, -1], D, p=[car, 0.8 - car, 0.05, 0.05, 0.05, 0.05]).astype(np.int32)
        im["gt_code"] = rng.choice([0, 1, 3, 4, 5, 9, 6], G, p=[0.6, 0.1, 0.1, 0.05, 0.05, 0.05, 0.05]).astype(np.int32)
        im["dt_height"] = rng.choice([20.0, 39.5, 40.0, 80.0], D, p=[0.05, 0.1, 0.35, 0.5])
        im["gt_height"] = rng.choice([20.0, 39.5, 40.0, 80.0, 120.0], G, p=[0.05, 0.1, 0.25, 0.3, 0.3])
        im["dt_score"] = rng.integers(0, 21, D) / 20.0
        im["gt_occ"] = rng.choice([0, 1, 2, 3], G, p=[0.8, 0.1, 0.05, 0.05]).astype(np.int32)
        im["gt_trunc"] = rng.choice([0.0, 0.0, 0.1, 0.15, 0.150001, 0.3], G)
        images.append(_sorted(im))
    for im in images:
        D, G = len(im["dt_code"]), len(im["gt_code"])
        im["gt_alpha"] = -rng.uniform(-np.pi, np.pi, G)                                  # (-pi, pi]
        im["dt_alpha"] = -rng.uniform(-np.pi, np.pi, D)
        if G:
            u, pick = rng.uniform(size=D), im["gt_alpha"][rng.integers(0, G, D)]
            im["dt_alpha"] = np.where(u < 0.25, pick, np.where(u < 0.42, pick + np.pi, im["dt_alpha"]))
        im["gt_alpha"][rng.uniform(size=G) < 0.1] = np.nan
        im["dt_alpha"][rng.uniform(size=D) < 0.1] = np.nan
    return images


def _per_image(images, c, d, m, alphas=True):
    out = []
    for im in images:
        row = TAB["cls_tab"][c]
        rel_g = [row[k] if 0 <= k < len(row) else -1 for k in im["gt_code"]]
        is_c = [0 <= k < len(row) and row[k] == 0 for k in im["dt_code"]]
        out.append({"sim": im["sim"][m].astype(np.float64), "score": im["dt_score"], "dc": im["dc"].astype(np.float64),
                    "gt_flag": X.gt_flags(rel_g, im["gt_height"], im["gt_occ"], im["gt_trunc"], TAB["diffs"][d]),
                    "dt_flag": X.dt_flags(is_c, im["dt_height"], TAB["diffs"][d][0]), "gt_alpha": im["gt_alpha"], "dt_alpha": im["dt_alpha"]})
    return out


@functools.lru_cache(maxsize=None)
def _oracle():
    images = _case()
    return [XA.evaluate_slot_aos(_per_image(images, c, d, m), TAB["min_ov"][o][c], use_dc=bool(TAB["dc_metric"][m])) for c, d, m, o in _slots(TAB)]


def test_oracle_counts_are_exact_kittis_and_the_inputs_have_what_the_test_is_about():
    images, ref = _case(), _oracle()
    assert len(images) == 257 and len(ref) == 3
    for (c, d, m, o), r in zip(_slots(TAB), ref):
        plain = X.evaluate_slot(_per_image(images, c, d, m), TAB["min_ov"][o][c], use_dc=bool(TAB["dc_metric"][m]))
        assert r["K"] == plain["K"] and r["thresholds"] == plain["thresholds"] and r["n_gt"] == plain["n_gt"]
        assert np.array_equal(r["counts"], plain["counts"]) and np.array_equal(r["precision"], plain["precision"])
        assert r["ap_r40"] == plain["ap_r40"] and r["ap_r11"] == plain["ap_r11"]
    r = ref[0]
    assert r["K"] >= 12 and 0.0 < r["aos_r40"] < r["ap_r40"] and 0.0 < r["aos_r11"] < r["ap_r11"], (r["K"], r["aos_r40"], r["ap_r40"])
    pairs = [(i, g, d) for per_image in r["pairs"] for i, ps in enumerate(per_image) for g, d in ps]
    assert any(np.isnan(images[i]["gt_alpha"][g]) for i, g, d in pairs) and any(np.isnan(images[i]["dt_alpha"][d]) for i, g, d in pairs)
    assert any(len(images[i]["dt_code"]) > 64 and d >= 64 for i, g, d in pairs)          # a true positive beyond the first lane round
    assert any(images[i]["gt_alpha"][g] == images[i]["dt_alpha"][d] for i, g, d in pairs)
    assert any(images[i]["dt_alpha"][d] == images[i]["gt_alpha"][g] + np.pi for i, g, d in pairs)
    assert {len(im["dt_code"]) for im in images} >= {0, 1, 63, 64, 65, 130, 1024} and {len(im["gt_code"]) for im in images} >= {0, 1, 40, 81}
    # one true positive a quarter turn off: q = 1 / 2
    one = [{"sim": np.array([[0.9]]), "score": [0.5], "dc": np.zeros((1, 0)), "gt_flag": [0], "dt_flag": [0], "gt_alpha": [0.25], "dt_alpha": [0.25 + np.pi / 2]}]
    r1 = XA.evaluate_slot_aos(one, 0.7)
    assert r1["K"] == 1 and abs(r1["aos"][0] - 0.5) <= 1e-15 and abs(int(r1["sim_fixed"][0]) - 2 ** 39) <= 1 and r1["precision"][0] == 1.0


def _alphas(images, dev, key):
    return torch.from_numpy(np.concatenate([im[key] for im in images] + [np.zeros(0)]).astype(np.float64)).to(dev)


def _launch(pb, dt_alpha, gt_alpha):
    """the five launches, every output poisoned first"""
    from omni3d_amd.kernels import kitti
    dev = pb.device
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=dev)          # noqa: E731
    junk = lambda dt, *s: torch.full(s, -77, dtype=dt, device=dev)                          # noqa: E731
    tp, n_gt = kitti.match_tp(pb)
    thr, K = kitti.thresholds(pb, tp, n_gt, 41)
    plain = kitti.match_counts(pb, thr, K)
    counts, sim_sum = kitti.match_counts_aos(pb, thr, K, dt_alpha, gt_alpha, AOS_METRIC, out=(junk(torch.int32, pb.S, 41, 3), junk(torch.int64, pb.S, 41)))
    assert torch.equal(counts, plain)                                                        # the bits of the plain entry point
    prec, rec, ap = kitti.finalize(pb, counts, K)
    aos, aos_ap = kitti.finalize_aos(pb, counts, sim_sum, K, AOS_METRIC, out=(nan(pb.S, 41), nan(pb.S, 2)))
    return {"tp_score": tp, "n_gt": n_gt, "thresholds": thr, "K": K, "counts": counts, "precision": prec, "recall": rec, "ap": ap,
            "sim_sum": sim_sum, "aos": aos, "aos_ap": aos_ap}


def _run(dev):
    from omni3d_amd.kernels import kitti
    images, ref = _case(), _oracle()
    pb = _problem(images, TAB, dev)
    dt_alpha, gt_alpha = _alphas(images, dev, "dt_alpha"), _alphas(images, dev, "gt_alpha")
    got = _launch(pb, dt_alpha, gt_alpha)
    again = kitti.run_aos(pb, dt_alpha, gt_alpha, AOS_METRIC)
    assert set(again) == set(got)
    for k in got:
        assert got[k].cpu().numpy().tobytes() == again[k].cpu().numpy().tobytes(), k           # two runs: the same bits (NaNs included)
    plain = kitti.run(pb)
    for k in plain:
        assert torch.equal(plain[k], again[k]), k
    h = {k: v.cpu().numpy() for k, v in got.items()}
    slots = _slots(TAB)
    worst_units, worst_aos = 0, 0.0
    for s, ((c, d, m, o), r) in enumerate(zip(slots, ref)):
        assert np.array_equal(h["counts"][s], r["counts"]) and h["K"][s] == r["K"], s
        if not AOS_METRIC[m]:
            assert not h["sim_sum"][s].any() and np.isnan(h["aos_ap"][s]).all() and np.isnan(h["aos"][s]).all(), s
            continue
        diff = np.abs(h["sim_sum"][s] - r["sim_fixed"])
        assert (diff <= h["counts"][s][:, 0]).all(), (s, diff.max())
        worst_units = max(worst_units, int(diff.max()))
        err = max(np.abs(h["aos"][s] - r["aos"]).max(), abs(h["aos_ap"][s, 0] - r["aos_r40"]), abs(h["aos_ap"][s, 1] - r["aos_r11"]))
        worst_aos = max(worst_aos, float(err))
        assert err <= 1e-9, (s, err)
        assert (h["aos"][s] <= h["precision"][s]).all() and (h["sim_sum"][s] >= 0).all() and not h["sim_sum"][s, r["K"]:].any()
    print("sim_sum: at most %d units from the oracle; aos / aos_ap: at most %.3g" % (worst_units, worst_aos))
    # all headings equal: every true positive adds exactly 2^40, AOS is AP
    same_d, same_g = torch.full_like(dt_alpha, 0.3), torch.full_like(gt_alpha, 0.3)
    eq = kitti.run_aos(pb, same_d, same_g, AOS_METRIC)
    for s, (c, d, m, o) in enumerate(slots):
        if AOS_METRIC[m]:
            assert torch.equal(eq["sim_sum"][s], eq["counts"][s, :, 0].long() * kitti.AOS_ONE)
            assert (eq["aos_ap"][s] - eq["ap"][s]).abs().max().item() <= 1e-9 and eq["ap"][s, 0].item() > 0
    # every detection half a turn from every ground truth: cos = -1 exactly, nothing is added
    opp = kitti.run_aos(pb, same_g.new_full(dt_alpha.shape, 0.3 + np.pi), same_g, AOS_METRIC)
    assert not opp["sim_sum"].any() and torch.equal(opp["counts"], plain["counts"])
    assert not opp["aos_ap"][[s for s, x in enumerate(slots) if AOS_METRIC[x[2]]]].any()
    # no metric asks for AOS: nothing accumulates, every slot is NaN
    none = kitti.run_aos(pb, dt_alpha, gt_alpha, (0, 0, 0))
    assert not none["sim_sum"].any() and torch.isnan(none["aos_ap"]).all() and torch.equal(none["counts"], plain["counts"])
    # arguments: ValueError before any launch
    thr, K = got["thresholds"], got["K"]
    for bad_d, bad_g, metric in ((dt_alpha.float(), gt_alpha, AOS_METRIC), (dt_alpha, gt_alpha[:-1], AOS_METRIC), (dt_alpha[None], gt_alpha, AOS_METRIC),
                                 (dt_alpha.tolist(), gt_alpha, AOS_METRIC), (dt_alpha, gt_alpha, (1, 0))):
        with pytest.raises(ValueError, match="alpha|aos_metric"):
            kitti.match_counts_aos(pb, thr, K, bad_d, bad_g, metric)
        with pytest.raises(ValueError, match="alpha|aos_metric"):
            kitti.run_aos(pb, bad_d, bad_g, metric)
    if dev != "cpu":
        with pytest.raises(ValueError, match="dt_alpha"):
            kitti.match_counts_aos(pb, thr, K, dt_alpha.cpu(), gt_alpha, AOS_METRIC)
    with pytest.raises(ValueError, match="sim_sum"):
        kitti.finalize_aos(pb, got["counts"], got["sim_sum"].int(), K, AOS_METRIC)
    # zero images and zero slots launch nothing
    empty = kitti.run_aos(_problem([], TAB, dev), dt_alpha[:0], gt_alpha[:0], AOS_METRIC)
    assert not empty["sim_sum"].any() and empty["aos_ap"][0].tolist() == [0.0, 0.0] and torch.isnan(empty["aos_ap"][1:]).all()


def test_aos_matching_emulated(emu_lib):
    _run("cpu")


@pytest.mark.gpu
def test_aos_matching_gpu(hip_lib):
    _run("cuda")


def test_row_limit_is_checked_before_anything_is_allocated():
    """2^23 ground-truth rows: sumG true positives of at most 2^40 units each could reach 2^63.  The launcher's argument check alone is
    asked, on a stand-in that holds nothing but the sizes."""
    from omni3d_amd.kernels import kitti
    assert kitti.AOS_MAX_ROWS == 2 ** 23 and kitti.AOS_ONE == 2 ** 40 and (kitti.AOS_MAX_ROWS - 1) * kitti.AOS_ONE < 2 ** 63
    with pytest.raises(ValueError, match="2\\^23"):
        kitti._check_aos(types.SimpleNamespace(sumG=2 ** 23, sumD=0, M=3, device=torch.device("cpu")), None, None, AOS_METRIC)
    with pytest.raises(ValueError, match="dt_alpha"):                              # one row fewer passes the size check and reaches the next one
        kitti._check_aos(types.SimpleNamespace(sumG=2 ** 23 - 1, sumD=0, M=3, device=torch.device("cpu")), None, None, AOS_METRIC)
