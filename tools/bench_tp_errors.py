"""Time of the true-positive error kernels (csrc/tp_errors.hip), run by hand on an MI355X; not part of bench.py.
 1. omni_pair_errors on 100 000 Omni3D-like pairs (`boxgen.omni3d_like_pairs`), the fits taken once beforehand (and timed on their
    own), outputs allocated once.
 2. omni_eval_tp_errors on a list of 50 categories x 20 000 detections x 4 depth ranges (hand-made match tables: about half of the
    detections are true positives, a tenth ignored), one wave per (category, range).
Device events around CALLS calls after 20 warm-up calls, repeated 5 times, the median reported with the spread and the clocks the
device reported right after the loops.  For scale only, the same work by the float64 test reference (tests/exact_tp_errors.py, numpy
and Python loops) on the host: the pair errors in full, the aggregation on one (category, range) list times 200.
Information only: there is no earlier figure and no speed bar.
    python tools/bench_tp_errors.py [output file]"""
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import exact_tp_errors  # noqa: E402
from omni3d_amd import boxgen, lib  # noqa: E402
from omni3d_amd.kernels import iou3d  # noqa: E402

PAIRS, WARMUP, REPEATS = 100_000, 20, 5
CATS, PER_CAT, RANGES = 50, 20_000, 4


def timed(call, calls):
    for _ in range(WARMUP):
        call()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            call()
        e1.record()
        torch.cuda.synchronize()
        out.append(1e3 * e0.elapsed_time(e1) / calls)
    return out


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


def match_tables(rng):
    """hand-made tables of CATS lists of PER_CAT detections: every detection has one candidate ground truth (pair_row = its index)"""
    sumD = CATS * PER_CAT
    kind = rng.uniform(size=(RANGES, sumD))
    dt_match = np.where(kind < 0.5, 0, -1).astype(np.int32)
    dt_ignore = (kind > 0.9).astype(np.uint8)
    order = np.concatenate([k * PER_CAT + rng.permutation(PER_CAT) for k in range(CATS)]).astype(np.int32)
    cat_off = (np.arange(CATS + 1) * PER_CAT).astype(np.int32)
    err = np.stack([rng.uniform(0, 2, sumD), rng.uniform(0, 1, sumD), rng.uniform(0, np.pi, sumD)], 1)
    npig = ((dt_match >= 0) & (dt_ignore == 0)).reshape(RANGES, CATS, PER_CAT).sum(-1).T.astype(np.int32) + 100
    return dict(order=order, cat_off=cat_off, dt_match=dt_match, dt_ignore=dt_ignore, pair_row=np.arange(sumD, dtype=np.int64), err=err,
                npig=np.ascontiguousarray(npig), has_e=np.ones(CATS, np.int32))


def main(out=None):
    assert torch.cuda.is_available(), "needs the GPU"
    rng = np.random.default_rng(0)
    dt_np, gt_np, _ = boxgen.omni3d_like_pairs(rng, PAIRS)
    dt, gt = torch.from_numpy(dt_np).cuda(), torch.from_numpy(gt_np).cuda()
    fit1, fit2 = iou3d.cuboid_fit(dt), iou3d.cuboid_fit(gt)
    idx = torch.arange(PAIRS, dtype=torch.int32, device="cuda")
    err = torch.empty((PAIRS, 3), dtype=torch.float64, device="cuda")
    L, st = lib.get(), lib.stream_of(dt)

    def pairs():
        L.call("omni_pair_errors", *[t.data_ptr() for t in fit1], PAIRS, *[t.data_ptr() for t in fit2], PAIRS, idx.data_ptr(), idx.data_ptr(),
               PAIRS, 0.0, 0.0, 0.0, err.data_ptr(), st)

    def fits():
        for boxes, fit in ((dt, fit1), (gt, fit2)):
            L.call("omni_cuboid_fit", boxes.data_ptr(), PAIRS, 1e-8, 1e-3, *[t.data_ptr() for t in fit], None, st)

    tab = match_tables(rng)
    dv = {k: torch.from_numpy(v).cuda() for k, v in tab.items()}
    thr_np = np.linspace(0.0, 1.0, 101)
    thr = torch.from_numpy(thr_np).cuda()
    tp_err = torch.full((CATS, RANGES, 3), -1.0, dtype=torch.float64, device="cuda")
    tp_cnt = torch.zeros((CATS, RANGES), dtype=torch.int32, device="cuda")
    sumD = CATS * PER_CAT

    def aggregate():
        L.call("omni_eval_tp_errors", dv["order"].data_ptr(), dv["cat_off"].data_ptr(), dv["dt_match"].data_ptr(), dv["dt_ignore"].data_ptr(),
               dv["pair_row"].data_ptr(), dv["err"].data_ptr(), sumD, dv["npig"].data_ptr(), dv["has_e"].data_ptr(), thr.data_ptr(), 0.1,
               CATS, RANGES, 101, sumD, tp_err.data_ptr(), tp_cnt.data_ptr(), st)

    t_pairs, t_fit, t_agg = timed(pairs, 2000), timed(fits, 2000), timed(aggregate, 200)
    during = clocks()
    # the results of the timed launches, checked against the reference
    t0 = time.perf_counter()
    want = exact_tp_errors.pair_errors(dt_np, gt_np, np.arange(PAIRS), np.arange(PAIRS))
    host_pairs = time.perf_counter() - t0
    got = err.cpu().numpy()
    ok = np.isfinite(want[:, 0])
    worst_pairs = float(np.abs(got[ok] - want[ok]).max())
    assert worst_pairs <= 1e-9 and np.array_equal(np.isfinite(got[:, 0]), ok), worst_pairs
    t0 = time.perf_counter()
    ds = [d for d in tab["order"][:PER_CAT] if not tab["dt_ignore"][0, d]]
    ref, cnt = exact_tp_errors.tp_aggregate([bool(tab["dt_match"][0, d] >= 0) for d in ds], [tab["err"][d] for d in ds if tab["dt_match"][0, d] >= 0],
                                            int(tab["npig"][0, 0]), thr_np, 0.1)
    host_agg = (time.perf_counter() - t0) * CATS * RANGES
    worst_agg = float(np.abs(tp_err[0, 0].cpu().numpy() - ref).max())
    assert worst_agg <= 2e-9 and int(tp_cnt[0, 0]) == cnt, worst_agg
    med_p, med_a = statistics.median(t_pairs), statistics.median(t_agg)
    lines = ["csrc/tp_errors.hip -- %d Omni3D-like pairs (%d with a valid fit on both sides), worst |kernel - float64 "
             "reference| over all of them %.1e" % (PAIRS, int(ok.sum()), worst_pairs),
             "omni_pair_errors: %s per call (%d x 2000 calls between device events after %d warm-up calls) = %.2f G pairs/s"
             % (fmt(t_pairs), REPEATS, WARMUP, PAIRS / med_p / 1e3),
             "omni_cuboid_fit, both sets (2 x %d boxes, two launches): %s" % (PAIRS, fmt(t_fit)),
             "omni_eval_tp_errors, %d categories x %d detections x %d ranges (%d waves), %d true positives in list (0, 0), worst |kernel - "
             "reference| there %.1e: %s per call (%d x 200 calls) = %.1f G detections/s"
             % (CATS, PER_CAT, RANGES, CATS * RANGES, cnt, worst_agg, fmt(t_agg), REPEATS, sumD * RANGES / med_a / 1e3),
             "for scale, the float64 test reference on the host (numpy and Python loops): pair errors with both fits %.1f s; aggregation "
             "%.1f s (one list timed, x %d)" % (host_pairs, host_agg, CATS * RANGES),
             "clocks right after the timed loops: %s" % during]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
