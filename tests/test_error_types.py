"""csrc/eval_errors.hip (`kernels.errtypes.error_types`, omni_eval_error_types) alone, on similarity matrices written by hand, against
`exact_errors.classify`: the definitions of `Omni3Deval.errors` in float64 with Python loops.  Type, attributed row, the three maxima,
the contest flags and the missed flags must be EQUAL to it: the kernel compares the float32 similarities as doubles, so on the same
float32 values there is nothing to round.

The data set of `_dataset` is one launch: an image with 130 detections and 70 ground truths over 3 categories (two LDS chunks, three
waves of detections) whose similarities are multiples of 1/16 -- so values exactly equal to t_fg = 0.5 and t_bg = 0.125, equal maxima
and, with scores out of eight values, tied contests occur (the run prints how many) --, an image without ground truth, one without detections, one
whose ground truths are all ignored, a small random one, and the hand-made image of `_hand_image`, whose expected codes are written out."""
import numpy as np
import pytest
import torch

import exact_errors as X

T_FG, T_BG = 0.5, 0.125


def _hand_image():
    """cats 0 / 1; ground truths: 0, 1 cat 0 free; 2 cat 0 matched; 3 cat 1 matched; 4 cat 1 free; 5 cat 0 ignored; 6 cat 1 free, untouched"""
    gt_cat, gt_matched, gt_ignore = [0, 0, 0, 1, 1, 0, 1], [0, 0, 1, 1, 0, 0, 0], [0, 0, 0, 0, 0, 1, 0]
    below = float(np.nextafter(np.float32(T_BG), np.float32(0)))
    rows = [                                               # (similarities to the seven ground truths, matched, ignored, score)
        ([0.9, 0, 0, 0, 0, 0, 0], 1, 0, 0.95),             # 0 TP
        ([0.9, 0, 0, 0, 0, 0, 0], 0, 1, 0.94),             # 1 IGN, whatever it overlaps
        ([T_BG, 0, 0.9, 0.9, 0, 0, 0], 0, 0, 0.90),        # 2 Loc on 0: s_free == t_bg pins the >=, and Loc precedes Cls and Dupe
        ([0.3, 0.3, 0, 0, 0, 0, 0], 0, 0, 0.50),           # 3 Loc on 1: two equal maxima, the later row
        ([0, 0.2, 0, 0, 0, 0, 0], 0, 0, 0.50),             # 4 Loc on 1 with the score of 3: the lower row (3) wins the contest
        ([0.1, 0, 0, T_FG, 0, 0, 0], 0, 0, 0.45),          # 5 Cls on 3 (s_other == t_fg), which is matched: removed by the oracle
        ([0, 0, 0, 0, 0.7, 0, 0], 0, 0, 0.40),             # 6 Cls on 4, which is free: wins
        ([0.1, 0, T_FG, 0.4, 0, 0, 0], 0, 0, 0.35),        # 7 Dupe on 2 (s_used == t_fg)
        ([0, 0.1, 0, 0, 0, 0.9, 0], 0, 0, 0.30),           # 8 Bkg: the ignored ground truth is no candidate
        ([0, 0, 0, 0.3, 0, 0, 0], 0, 0, 0.25),             # 9 Both: t_bg <= 0.3 < t_fg on another category
        ([below, 0, 0, 0, 0, 0, 0], 0, 0, 0.20),           # 10 Bkg: one float32 step below t_bg pins the <
    ]
    img = {"sim": np.array([r[0] for r in rows], np.float32), "dt_cat": [0] * len(rows), "dt_matched": [r[1] for r in rows],
           "dt_ignore": [r[2] for r in rows], "dt_score": [r[3] for r in rows], "gt_cat": gt_cat, "gt_matched": gt_matched, "gt_ignore": gt_ignore}
    want = {"type": [X.TP, X.IGN, X.LOC, X.LOC, X.LOC, X.CLS, X.CLS, X.DUPE, X.BKG, X.BOTH, X.BKG], "attr": [-1, -1, 0, 1, 1, 3, 4, 2, -1, -1, -1],
            "win_loc": [0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0], "win_cls": [0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0], "missed": [0, 0, 0, 0, 0, 0, 1]}
    return img, want


def _random_image(rng, D, G, cats=3, all_ignored=False):
    sim = (rng.integers(0, 10, (D, G)) / 16.0).astype(np.float32)
    sim[rng.uniform(size=(D, G)) < 0.8] = 0.0
    return {"sim": sim, "dt_cat": rng.integers(0, cats, D).tolist(), "dt_matched": (rng.uniform(size=D) < 0.2).astype(int).tolist(),
            "dt_ignore": (rng.uniform(size=D) < 0.1).astype(int).tolist(), "dt_score": (rng.integers(1, 9, D) / 8.0).tolist(),
            "gt_cat": rng.integers(0, cats, G).tolist(), "gt_matched": (rng.uniform(size=G) < 0.4).astype(int).tolist(),
            "gt_ignore": [1] * G if all_ignored else (rng.uniform(size=G) < 0.15).astype(int).tolist()}


def _dataset():
    rng = np.random.default_rng(5)
    hand, want = _hand_image()
    return [_random_image(rng, 130, 70), _random_image(rng, 7, 0), _random_image(rng, 0, 5), _random_image(rng, 9, 6, all_ignored=True),
            _random_image(rng, 12, 9), hand], want


def _launch(images, dev, t_fg=T_FG, t_bg=T_BG):
    from omni3d_amd.kernels import errtypes
    cat = lambda key, dt: torch.from_numpy(np.concatenate([np.asarray(im[key], dt).reshape(-1) for im in images])).to(dev)      # noqa: E731
    off = lambda key: torch.from_numpy(np.concatenate([[0], np.cumsum([len(im[key]) for im in images])]).astype(np.int32)).to(dev)   # noqa: E731
    return errtypes.error_types(cat("sim", np.float32), off("dt_cat"), off("gt_cat"), cat("dt_cat", np.int32), cat("dt_matched", np.uint8),
                                cat("dt_ignore", np.uint8), cat("dt_score", np.float64), cat("gt_cat", np.int32), cat("gt_matched", np.uint8),
                                cat("gt_ignore", np.uint8), t_fg, t_bg)


def _run_kernel(dev):
    from omni3d_amd.kernels import errtypes
    assert (errtypes.TP, errtypes.IGN, errtypes.CLS, errtypes.LOC, errtypes.BOTH, errtypes.DUPE, errtypes.BKG) == \
        (X.TP, X.IGN, X.CLS, X.LOC, X.BOTH, X.DUPE, X.BKG)
    images, want = _dataset()
    got = {k: v.cpu().numpy() for k, v in _launch(images, dev).items()}
    again = {k: v.cpu().numpy() for k, v in _launch(images, dev).items()}
    for k in got:                                                                   # two runs, bit for bit
        assert got[k].tobytes() == again[k].tobytes(), k
    assert got["type"].dtype == np.int8 and got["attr"].dtype == np.int32 and got["smax"].dtype == np.float32
    d0 = g0 = 0
    seen, ties, at_thr = set(), 0, 0
    for n, im in enumerate(images):
        D, G = len(im["dt_cat"]), len(im["gt_cat"])
        ref = X.classify(im["sim"].astype(np.float64), im["dt_cat"], im["dt_matched"], im["dt_ignore"], im["dt_score"], im["gt_cat"],
                         im["gt_matched"], im["gt_ignore"], T_FG, T_BG)
        ds, gs = slice(d0, d0 + D), slice(g0, g0 + G)
        assert np.array_equal(got["type"][ds], ref["type"]), n
        assert np.array_equal(got["attr"][ds], np.where(ref["attr"] >= 0, ref["attr"] + g0, -1)), n
        assert np.array_equal(got["smax"][ds].astype(np.float64), ref["smax"]), n   # -inf for an empty set included
        assert np.array_equal(got["win_loc"][ds].astype(bool), ref["win_loc"]) and np.array_equal(got["win_cls"][ds].astype(bool), ref["win_cls"]), n
        assert np.array_equal(got["gt_missed"][gs].astype(bool), ref["missed"]), n
        seen |= set(ref["type"].tolist())
        for code in (X.LOC, X.CLS):                                                 # contests decided by the row alone
            for g in range(G):
                rows = [d for d in range(D) if ref["type"][d] == code and ref["attr"][d] == g]
                ties += len(rows) > 1 and sorted(im["dt_score"][d] for d in rows)[-1] == sorted(im["dt_score"][d] for d in rows)[-2]
        fp = ~np.isin(ref["type"], (X.TP, X.IGN))
        at_thr += int(((ref["smax"][fp] == T_FG) | (ref["smax"][fp] == T_BG)).sum())
        d0, g0 = d0 + D, g0 + G
    print("tied contests %d, maxima of false positives exactly at a threshold %d" % (ties, at_thr))
    assert seen == set(range(7)) and ties >= 3 and at_thr >= 8
    big = X.classify(images[0]["sim"].astype(np.float64), *[images[0][k] for k in ("dt_cat", "dt_matched", "dt_ignore", "dt_score", "gt_cat",
                                                                                  "gt_matched", "gt_ignore")], T_FG, T_BG)
    assert big["win_loc"].sum() >= 5 and big["win_cls"].sum() >= 2 and big["missed"].sum() >= 2
    assert (got["type"][130:137][~np.isin(got["type"][130:137], (X.TP, X.IGN))] == X.BKG).all()        # no ground truth: all Bkg
    assert (got["type"][137:146][~np.isin(got["type"][137:146], (X.TP, X.IGN))] == X.BKG).all()        # all ignored: all Bkg
    assert not got["gt_missed"][75:81].any() and np.isinf(got["smax"][137:146]).all()
    # the hand-made image, against the codes written out
    hd, hg = slice(d0 - 11, d0), slice(g0 - 7, g0)
    assert got["type"][hd].tolist() == want["type"]
    assert np.where(got["attr"][hd] >= 0, got["attr"][hd] - (g0 - 7), -1).tolist() == want["attr"]
    assert got["win_loc"][hd].tolist() == want["win_loc"] and got["win_cls"][hd].tolist() == want["win_cls"]
    assert got["gt_missed"][hg].tolist() == want["missed"]
    # an empty data set is legal
    empty = _launch([_random_image(np.random.default_rng(0), 0, 0)], dev)
    assert all(v.numel() == 0 for v in empty.values())


def test_error_types_emulated(emu_lib):
    _run_kernel("cpu")


@pytest.mark.gpu
def test_error_types_gpu(hip_lib):
    _run_kernel("cuda")


def _run_refusals(dev, lib):
    """capacity + 1 ground truths, thresholds out of order: ValueError from the wrapper, OMNI_ERR_ARG from the library, nothing launched"""
    from omni3d_amd.kernels import errtypes
    from omni3d_amd.lib import OmniHipError
    rng = np.random.default_rng(1)
    _launch([_random_image(rng, 2, errtypes.MAX_GT)], dev)                          # the capacity itself is fine
    with pytest.raises(ValueError, match="capacity"):
        _launch([_random_image(rng, 2, 3), _random_image(rng, 0, errtypes.MAX_GT + 1)], dev)
    for t_fg, t_bg in ((0.5, 0.5), (0.5, 0.0), (0.1, 0.5), (float("nan"), 0.1)):
        with pytest.raises(ValueError):
            _launch([_random_image(rng, 2, 3)], dev, t_fg, t_bg)
    fake = 1 << 20                                                                  # never dereferenced: the check comes first
    for max_gt, t_bg in ((errtypes.MAX_GT + 1, 0.1), (4, 0.6), (4, float("nan"))):
        with pytest.raises(OmniHipError, match="status 1"):
            lib.call("omni_eval_error_types", *([fake] * 11), 0.5, t_bg, 1, 4, 4, max_gt, *([fake] * 6), None)
    good = _random_image(rng, 4, 3)
    for key, value in (("dt_cat", [0, 1, 2]), ("gt_ignore", [0] * 4)):
        with pytest.raises(ValueError):
            _launch([{**good, key: value}], dev)


def test_refusals_emulated(emu_lib):
    _run_refusals("cpu", emu_lib)


@pytest.mark.gpu
def test_refusals_gpu(hip_lib):
    _run_refusals("cuda", hip_lib)


def test_header_declares_the_entry():
    from omni3d_amd import lib
    assert lib.parse_header()["omni_eval_error_types"] == "p" * 11 + "dd" + "iiii" + "p" * 7
    text = open(lib.HEADER_PATH).read()
    assert "TIDE" in text and "no call site" in text
