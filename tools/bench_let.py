"""Time of the longitudinal-error-tolerant kernels (csrc/let_iou.hip), run by hand on an MI355X; not part of bench.py.
 1. omni_let_pairs on 100 000 Omni3D-like pairs (`boxgen.omni3d_like_pairs`), next to omni_iou3d_exact_pairs (csrc/iou3d_exact.hip) on the
same pairs: the sibling does the same clipping without the alignment, so it is the number to judge against.  The fits are taken once
beforehand, the outputs allocated once.  Device events around CALLS calls after 20 warm-up calls; the two kernels alternate, 5 blocks
each, the medians and the spread are reported with the clocks the device reported right after the loops.  The results of the timed
launches are checked against the float64 test reference (tests/exact_let.py): aff and lon on all pairs, let_iou on the first 300 with
aff > 0; let_iou lies in [0, 1] and is exactly 0 where aff is 0.
 2. omni_eval_accumulate_let next to omni_eval_accumulate (csrc/eval_match.hip) on the same hand-made tables: 20 categories x 10 000
detections x 4 depth ranges x 3 maxDets x 10 thresholds (2 400 waves; about half of the detections are true positives, a tenth
ignored), alternating blocks as above; category 0 is checked against the reference.
Information only: no speed bar is fixed in advance.
    python tools/bench_let.py [output file]"""
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import exact_let  # noqa: E402
from omni3d_amd import boxgen, lib  # noqa: E402
from omni3d_amd.kernels import iou3d  # noqa: E402

PAIRS, WARMUP, BLOCKS, CALLS = 100_000, 20, 5, 500
CHECK_IOU = 300
CATS, PER_CAT, RANGES, THRS, MAX_DETS, ACC_CALLS = 20, 10_000, 4, 10, (1, 10, 100), 50


def match_tables(rng):
    """hand-made tables of CATS lists of PER_CAT detections: every detection has one candidate ground truth (pair_row = its index);
    ranks 0 .. 124, so that every maxDets cuts the lists differently"""
    sumD = CATS * PER_CAT
    kind = rng.uniform(size=(RANGES, THRS, sumD))
    dt_match = np.where(kind < 0.5, 0, -1).astype(np.int32)
    dt_ignore = (kind > 0.9).astype(np.uint8)
    score = rng.uniform(size=sumD)
    cat = np.repeat(np.arange(CATS), PER_CAT)
    order = np.lexsort((np.arange(sumD), -score, cat)).astype(np.int32)
    npig = ((dt_match[:, 0] >= 0) & (dt_ignore[:, 0] == 0)).reshape(RANGES, CATS, PER_CAT).sum(-1).T.astype(np.int32) + 100
    return dict(order=order, cat_off=(np.arange(CATS + 1) * PER_CAT).astype(np.int32), rank=rng.integers(0, 125, sumD).astype(np.int32),
                score=score, dt_match=dt_match, dt_ignore=dt_ignore, pair_row=np.arange(sumD, dtype=np.int64), aff=rng.uniform(0, 1, sumD),
                lon=rng.normal(0, 1, sumD), npig=np.ascontiguousarray(npig), has_e=np.ones(CATS, np.int32),
                max_dets=np.array(MAX_DETS, np.int32), rec_thrs=np.linspace(0.0, 1.0, 101))


def clocks():
    """the sclk / mclk lines of `rocm-smi --showclocks` (read only), or a note that they could not be read"""
    try:
        text = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        rows = [" ".join(ln.split()) for ln in text.splitlines() if "sclk" in ln or "mclk" in ln]
        return "; ".join(rows[:2]) if rows else "clocks not reported"
    except Exception as exc:      # noqa: BLE001
        return "clocks not read (%s)" % type(exc).__name__


def fmt(t):
    return "median %.1f us (min %.1f, max %.1f)" % (statistics.median(t), min(t), max(t))


def block(call, calls=CALLS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        call()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / calls


def main(out=None):
    assert torch.cuda.is_available(), "needs the GPU"
    rng = np.random.default_rng(0)
    dt_np, gt_np, _ = boxgen.omni3d_like_pairs(rng, PAIRS)
    dt, gt = torch.from_numpy(dt_np).cuda(), torch.from_numpy(gt_np).cuda()
    fit1, fit2 = iou3d.cuboid_fit(dt), iou3d.cuboid_fit(gt)
    idx = torch.arange(PAIRS, dtype=torch.int32, device="cuda")
    iou = torch.empty(PAIRS, dtype=torch.float32, device="cuda")
    aff, lon = torch.empty(PAIRS, dtype=torch.float64, device="cuda"), torch.empty(PAIRS, dtype=torch.float64, device="cuda")
    vol, iou_x = torch.empty(PAIRS, dtype=torch.float32, device="cuda"), torch.empty(PAIRS, dtype=torch.float32, device="cuda")
    L, st = lib.get(), lib.stream_of(dt)
    f1, f2 = [t.data_ptr() for t in fit1], [t.data_ptr() for t in fit2]

    def let_pairs():
        L.call("omni_let_pairs", *f1, PAIRS, *f2, PAIRS, idx.data_ptr(), idx.data_ptr(), PAIRS, 0.1, 0.5, iou.data_ptr(), aff.data_ptr(),
               lon.data_ptr(), st)

    def exact_pairs():
        L.call("omni_iou3d_exact_pairs", *f1, PAIRS, *f2, PAIRS, idx.data_ptr(), idx.data_ptr(), PAIRS, vol.data_ptr(), iou_x.data_ptr(), st)

    for _ in range(WARMUP):
        let_pairs()
        exact_pairs()
    torch.cuda.synchronize()
    t_let, t_exact = [], []
    for _ in range(BLOCKS):                                        # alternating: both see the same clocks and neighbours
        t_let.append(block(let_pairs))
        t_exact.append(block(exact_pairs))
    # ---- the accumulation
    tab = match_tables(rng)
    dv = {k: torch.from_numpy(v).cuda() for k, v in tab.items()}
    K, A, M, T, R, sumD = CATS, RANGES, len(MAX_DETS), THRS, 101, CATS * PER_CAT
    full = lambda shape: torch.full(shape, -1.0, dtype=torch.float64, device="cuda")      # noqa: E731
    prec, rec, scr = full((T, R, K, A, M)), full((T, K, A, M)), full((T, R, K, A, M))
    prec_l, tp_aff, tp_lon = full((T, R, K, A, M)), full((T, K, A, M)), full((T, K, A, M))
    p = {k: v.data_ptr() for k, v in dv.items()}

    def accumulate():
        L.call("omni_eval_accumulate", p["order"], p["cat_off"], p["rank"], p["score"], p["dt_match"], p["dt_ignore"], p["npig"], p["has_e"],
               p["rec_thrs"], p["max_dets"], K, A, M, T, R, sumD, prec.data_ptr(), rec.data_ptr(), scr.data_ptr(), st)

    def accumulate_let():
        L.call("omni_eval_accumulate_let", p["order"], p["cat_off"], p["rank"], p["dt_match"], p["dt_ignore"], p["pair_row"], p["aff"], p["lon"],
               sumD, p["npig"], p["has_e"], p["rec_thrs"], p["max_dets"], K, A, M, T, R, sumD, prec_l.data_ptr(), tp_aff.data_ptr(),
               tp_lon.data_ptr(), st)

    for _ in range(3):
        accumulate_let()
        accumulate()
    torch.cuda.synchronize()
    t_accl, t_acc = [], []
    for _ in range(BLOCKS):
        t_accl.append(block(accumulate_let, ACC_CALLS))
        t_acc.append(block(accumulate, ACC_CALLS))
    during = clocks()
    only0 = np.zeros(CATS, np.int32)
    only0[0] = 1
    want = exact_let.accumulate(tab["order"], tab["cat_off"], tab["rank"], tab["dt_match"], tab["dt_ignore"], tab["pair_row"], tab["aff"],
                                tab["lon"], tab["npig"], only0, tab["rec_thrs"], list(MAX_DETS))
    worst_acc = max(float(np.abs(got.cpu().numpy()[..., 0, :, :] - want[key][..., 0, :, :]).max())
                    for got, key in ((prec_l, "precision_l"), (tp_aff, "tp_affinity"), (tp_lon, "tp_lon"), (prec, "precision")))
    assert worst_acc <= 2e-9, worst_acc
    assert bool((prec_l <= prec + 2e-9).all())
    # the results of the timed launches
    g_iou, g_aff, g_lon, g_x = iou.cpu().numpy(), aff.cpu().numpy(), lon.cpu().numpy(), iou_x.cpu().numpy()
    _, w_aff, w_lon = exact_let.let_pairs(dt_np, gt_np, np.arange(PAIRS), np.arange(PAIRS), iou=False)
    gated = np.isnan(w_lon)
    assert np.array_equal(np.isnan(g_lon), gated) and not np.isnan(g_iou).any() and not np.isnan(g_aff).any()
    worst_aff, worst_lon = float(np.abs(g_aff - w_aff).max()), float(np.abs(g_lon[~gated] - w_lon[~gated]).max())
    assert worst_aff <= 1e-9 and worst_lon <= 1e-9, (worst_aff, worst_lon)
    assert (g_iou >= 0).all() and (g_iou <= 1).all() and (g_iou[g_aff == 0] == 0).all()
    some = np.flatnonzero(w_aff > 0)[:CHECK_IOU]
    w_iou = exact_let.let_pairs(dt_np[some], gt_np[some], np.arange(len(some)), np.arange(len(some)))[0]
    worst_iou = float(np.abs(g_iou[some] - w_iou).max())
    assert worst_iou <= 1e-5, worst_iou
    med_l, med_x = statistics.median(t_let), statistics.median(t_exact)
    med_al, med_a = statistics.median(t_accl), statistics.median(t_acc)
    lines = ["csrc/let_iou.hip -- %d Omni3D-like pairs: %d gated (invalid box), %d with aff == 0 (no clipping), %d clipped, %d with "
             "LET-IoU > 0 (plain exact IoU > 0: %d)" % (PAIRS, int(gated.sum()), int(((g_aff == 0) & ~gated).sum()), int((g_aff > 0).sum()),
                                                       int((g_iou > 0).sum()), int((g_x > 0).sum())),
             "worst |kernel - float64 reference|: aff %.1e, lon %.1e over all pairs; let_iou %.1e over the first %d with aff > 0"
             % (worst_aff, worst_lon, worst_iou, len(some)),
             "omni_let_pairs:         %s per call = %.1f M pairs/s" % (fmt(t_let), PAIRS / med_l),
             "omni_iou3d_exact_pairs: %s per call = %.1f M pairs/s, the same pairs" % (fmt(t_exact), PAIRS / med_x),
             "    let / exact = %.2f (%d alternating blocks of %d calls between device events after %d warm-up calls of each)"
             % (med_l / med_x, BLOCKS, CALLS, WARMUP),
             "omni_eval_accumulate_let, %d categories x %d detections x %d ranges x %d maxDets x %d thresholds (%d waves), worst |kernel - "
             "reference| on category 0 %.1e: %s per call" % (CATS, PER_CAT, RANGES, len(MAX_DETS), THRS, K * A * M * T, worst_acc, fmt(t_accl)),
             "omni_eval_accumulate on the same tables: %s per call" % fmt(t_acc),
             "    let / plain = %.2f (%d alternating blocks of %d calls)" % (med_al / med_a, BLOCKS, ACC_CALLS),
             "clocks right after the timed loops: %s" % during]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
