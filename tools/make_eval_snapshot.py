"""Characterisation snapshot of the Python evaluator: what `Omni3Deval`, `_derive_results`, the four `*_groups` pair passes and the
short form of `Omni3DEvaluator` give on one fixed scene, in all five modes, down to the bytes of every table and the order of the
kernel launches.  tests/test_eval_snapshot.py re-runs `record()` and asks for equality with the file written here, so a change to the
evaluator's Python that moves a result, a printed line or a launch shows up.

    python tools/make_eval_snapshot.py [--target emu|gfx950] [--out FILE]      write tests/golden/eval_snapshot_<target>.json
    python tools/make_eval_snapshot.py [--target ...] --time                   host time of evaluate + accumulate + summarize per mode

The scene is `tests/bootstrap_scene.scene()` (6 images, 3 categories, 130 detections in category 1, 14 in one image, `ignore3D`, all
depth ranges) with, on a copy, one detection's `bbox3D` collapsed to a point so that the warnings fire.  Per mode: evaluate /
accumulate / summarize, `_derive_results`, `bootstrap(n=8, seed=0)`, and a second pass with proximity evaluation on two images.  Small
things are stored verbatim (floats as their repr, so NaN compares), arrays as shape, dtype and sha256 of their bytes, and per phase the
names handed to `HipLibrary.call`.  target `emu` = the host-emulated kernels of tests/hipemu, `gfx950` = the real library."""
import argparse
import contextlib
import copy
import hashlib
import io
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

MODES = ("2D", "3D", "BEV", "DIST", "LET")
SECTIONS = MODES + ("groups", "short_form")
DEGENERATE_DT = 5                       # index of the detection whose cuboid is collapsed
PROX_IMGS = (16, 48)                    # the second pass: proximity evaluation on these two images only
EXTRA_PAIR = ("pair_err", "pair_aff", "pair_lon")
SHORT_KW = dict(eval_bev=True, eval_dist=True, dist_up=(0.0, -1.0, 0.0), dist_params={"distThrs": [0.5, 1.0, 2.0, 4.0, 8.0], "tpDist": 1.0},
                eval_let=True, let_params={"lonTolMin": 1.0}, bootstrap={"n": 8, "seed": 0})


def snapshot_path(target):
    return os.path.join(ROOT, "tests", "golden", "eval_snapshot_%s.json" % target)


def altered_scene():
    import bootstrap_scene as S
    gts, dts = copy.deepcopy(S.scene())
    dts[DEGENERATE_DT]["bbox3D"] = [dts[DEGENERATE_DT]["bbox3D"][0]] * 8
    return gts, dts, list(S.IMGS), list(S.CATS)


def _num(v):
    return repr(float(v))


def _nums(a):
    return [_num(v) for v in np.asarray(a, dtype=np.float64).reshape(-1)]


def _digest(a):
    a = a.detach().cpu().contiguous().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return {"shape": list(a.shape), "dtype": str(a.dtype), "sha256": hashlib.sha256(a.tobytes()).hexdigest()}


@contextlib.contextmanager
def _phase(lib, into, name):
    """stdout and the names given to `lib.call` while the block runs -> into[name]"""
    calls, out, real = [], io.StringIO(), lib.call
    lib.call = lambda fn, *args: (calls.append(fn), real(fn, *args))[1]
    try:
        with contextlib.redirect_stdout(out):
            yield
    finally:
        del lib.call
    into[name] = {"calls": calls, "stdout": out.getvalue()}


def _make(E, gts, dts, imgs, cats, mode, **kw):
    return E.Omni3Deval(E.AnnotationIndex(copy.deepcopy(gts), imgs, cats), E.AnnotationIndex(copy.deepcopy(dts), imgs, cats), mode=mode, **kw)


def _three_steps(lib, E, ev, rec):
    with _phase(lib, rec, "evaluate"):
        ev.evaluate()
    with _phase(lib, rec, "accumulate"):
        ev.accumulate()
    with _phase(lib, rec, "summarize"):
        text = ev.summarize()
    rec["summary"] = text
    rec["stats"] = _nums(ev.stats)
    for name in ("tp_stats", "stats_l", "let_stats"):
        if hasattr(ev, name):
            rec[name] = _nums(getattr(ev, name))
    rec["eval"] = {k: (_digest(v) if isinstance(v, np.ndarray) else v) for k, v in ev.eval.items() if k not in ("params", "date")}
    rec["match"] = {k: _digest(v) for k, v in ev._dev["match"].items()}
    rec["pair"] = {k: _digest(ev._dev[k]) for k in EXTRA_PAIR if k in ev._dev}


def _record_mode(lib, E, mode):
    gts, dts, imgs, cats = altered_scene()
    rec = {}
    ev = _make(E, gts, dts, imgs, cats, mode)
    _three_steps(lib, E, ev, rec)
    with _phase(lib, rec, "derive"):
        derived = E._derive_results(ev, mode, ["cat%d" % c for c in cats])
    rec["derived"] = [[k, _num(v)] for k, v in derived.items()]
    with _phase(lib, rec, "bootstrap"):
        bs = ev.bootstrap(n=8, seed=0)
    rec["bootstrap_ci"], rec["bootstrap_point"] = _nums(bs["ci"]), _nums(bs["point"])
    rec["prox"] = {}
    _three_steps(lib, E, _make(E, gts, dts, imgs, cats, mode, eval_prox=set(PROX_IMGS)), rec["prox"])
    return rec


def _record_groups(lib, E):
    """the four pair passes called directly with warn=True, on the scene's boxes in (category, image) groups"""
    gts, dts, imgs, cats = altered_scene()
    keys = [(c, i) for c in cats for i in imgs]
    d_by = {k: [d for d in dts if (d["category_id"], d["image_id"]) == k] for k in keys}
    g_by = {k: [g for g in gts if (g["category_id"], g["image_id"]) == k] for k in keys}
    dev = "cpu" if lib.emulated else "cuda"
    t = lambda recs: torch.tensor(np.asarray([r["bbox3D"] for r in recs], np.float32).reshape(-1, 8, 3)).to(dev)      # noqa: E731
    b_d, b_g = t([d for k in keys for d in d_by[k]]), t([g for k in keys for g in g_by[k]])
    ds, gs = [len(d_by[k]) for k in keys], [len(g_by[k]) for k in keys]
    rec = {}
    for name in ("box3d_overlap_groups", "bev_overlap_groups", "dist_errors_groups", "let_overlap_groups"):
        with _phase(lib, rec, name):
            out = getattr(E, name)(b_d, b_g, ds, gs, warn=True)
        flats = [torch.cat([m.reshape(-1) for m in out])] if isinstance(out, list) else [o for o in out if isinstance(o, torch.Tensor)]
        views = out if isinstance(out, list) else out[-1]
        rec[name].update(flat=[_digest(f) for f in flats], views=[list(v.shape) for v in views])
    return rec


def _record_short(lib, E):
    gts, dts, imgs, cats = altered_scene()
    rec = {}
    ev = E.Omni3DEvaluator(copy.deepcopy(gts), imgs, cats, False, **SHORT_KW)
    ev.process([{"image_id": i} for i in imgs], [{"instances": [copy.deepcopy(d) for d in dts if d["image_id"] == i]} for i in imgs])
    with _phase(lib, rec, "evaluate"):
        res = ev.evaluate()["bbox"]
    rec["keys"] = list(res)
    rec["values"] = [[k, _nums(v)] for k, v in res.items() if not k.startswith("omni_eval_")]
    rec["stats"] = [[k, _nums(v.stats)] for k, v in res.items() if k.startswith("omni_eval_")]
    return rec


def record_section(lib, name):
    """-> one section of the snapshot (a JSON-able dict): a mode of MODES, "groups" or "short_form"; `lib` must be the installed library"""
    from omni3d_amd.cubercnn.evaluation import omni3d_evaluation as E
    rec = _record_mode(lib, E, name) if name in MODES else {"groups": _record_groups, "short_form": _record_short}[name](lib, E)
    return json.loads(json.dumps(rec))


def record(lib):
    return {name: record_section(lib, name) for name in SECTIONS}


def measure(lib, runs=20, warmup=3):
    """-> {mode: (median, min, max)} wall milliseconds of evaluate + accumulate + summarize on the scene"""
    from omni3d_amd.cubercnn.evaluation import omni3d_evaluation as E
    gts, dts, imgs, cats = altered_scene()
    out = {}
    for mode in MODES:
        times = []
        for k in range(warmup + runs):
            ev = _make(E, gts, dts, imgs, cats, mode)
            with contextlib.redirect_stdout(io.StringIO()):
                t0 = time.perf_counter()
                ev.evaluate()
                ev.accumulate()
                ev.summarize()
                if not lib.emulated:
                    torch.cuda.synchronize()
                t1 = time.perf_counter()
            if k >= warmup:
                times.append(1e3 * (t1 - t0))
        out[mode] = (statistics.median(times), min(times), max(times))
    return out


def dumps(obj, depth=3, indent=""):
    """JSON with one line per entry down to `depth` levels of dicts, compact below: a diff of two snapshots stays readable"""
    if depth == 0 or not isinstance(obj, dict) or not obj:
        return json.dumps(obj)
    inner = indent + " "
    return "{\n" + ",\n".join(inner + json.dumps(k) + ": " + dumps(v, depth - 1, inner) for k, v in obj.items()) + "\n" + indent + "}"


def install(target):
    from omni3d_amd import lib as L
    if target == "emu":
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hipemu"), "-j8"])
        L._install_for_tests(L.HipLibrary(os.path.join(ROOT, "tests", "hipemu", "libomni3d_emu.so"), emulated=True))
    else:
        L._install_for_tests(None)
    return L.get()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--target", choices=["emu", "gfx950"], default="gfx950" if torch.cuda.is_available() else "emu")
    ap.add_argument("--out", default=None)
    ap.add_argument("--time", action="store_true", help="print the host time per mode and write nothing")
    args = ap.parse_args(argv)
    lib = install(args.target)
    if args.time:
        for mode, (med, lo, hi) in measure(lib).items():
            print("target=%s mode=%-4s evaluate+accumulate+summarize: median %.3f ms  min %.3f  max %.3f  (20 runs after 3)" % (args.target, mode, med, lo, hi))
        return
    path = args.out or snapshot_path(args.target)
    with open(path, "w") as f:
        f.write(dumps(record(lib)) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
