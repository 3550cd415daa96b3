"""The mode table of the evaluator: one object per evaluation mode in `MODES`, and everything that differs by mode -- nothing else in
this package compares a mode against a name.

A new mode derives from `Mode3D`, overrides the hooks it changes (every one has a no-op or 2D / 3D default) and is listed in `MODES`;
DESIGN.md ("Adding an evaluation mode") lists the hooks in the order an evaluation meets them.  `enabled_modes` maps the drivers'
public switches to the list of modes of a run, `check_options` checks their other keywords."""
import numpy as np
import torch

from ...kernels import let, tperr
from .pairs import BEV_UP, _pair_index, _xywh_iou

_LET_TP_IOU = 0.25                         # the threshold at which summarize() reports mean affinity and longitudinal error
_TP_NAMES = ("ATE", "ASE", "AOE")          # metres, 1 - IoU of the aligned boxes, radians: not scaled by 100


def _mean(values):
    values = list(values)
    return float(np.mean(values)) if values else float("nan")


def _percent(v):
    return float(v * 100 if v >= 0 else "nan")


def _table_ap(table, k):
    """mean of a (T, R, K, A, M) table over thresholds and recall points for category k at range 'all', the largest maxDets (x100)"""
    vals = table[:, :, k, 0, -1]
    vals = vals[vals > -1]
    return float(np.mean(vals) * 100) if vals.size else float("nan")


def _ap_columns(label, r, categories, metrics, ap="AP"):
    """`label` = mean of the per-category APs like AP3D, then the six headline columns ('AP15' -> label@15, 'APn' -> label-N)"""
    out = {label: _mean(r[ap + "-" + c] for c in categories if ap + "-" + c in r)}
    out.update({label + "@" + m[2:].lstrip("@"): r[m.replace("AP", ap, 1)] for m in metrics[1:4]})
    out.update({label + "-" + m[-1].upper(): r[m.replace("AP", ap, 1)] for m in metrics[4:]})
    return out


class Mode2D:
    """the COCO protocol on the 2D boxes (reference omni3d_evaluation.py:1019-1088 for the params)"""
    name = "2D"
    ignore_key, box_key, range_key, box_shape = "ignore2D", "bbox", "area", (-1, 4)
    iou_range, area_lbl = (0.5, 0.95), ["all", "small", "medium", "large"]
    area_rng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
    thresholds, shown = [0.5, 0.75, 0.95], "iouThrs"
    fmt = " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}"
    metrics = ["AP", "AP50", "AP75", "AP95", "APs", "APm", "APl"]
    switch, up_option, extension, results, concat_ci = None, "bev_up", False, None, True
    options = {"bev_up": lambda up: tuple(float(v) for v in up)}
    # `Omni3Deval.errors`: the default (t_fg, t_bg) -- conventions, not tuned values: TIDE's -- and whether `loc_errors` applies
    error_thrs, loc_errors = (0.5, 0.1), False

    def set_params(self, p):
        lo, hi = self.iou_range
        p.imgIds, p.catIds = [], []
        p.iouThrs = np.linspace(lo, hi, int(np.round((hi - lo) / 0.05)) + 1, endpoint=True)
        p.recThrs = np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True)
        p.maxDets = [1, 10, 100]
        p.areaRng, p.areaRngLbl = [list(r) for r in self.area_rng], list(self.area_lbl)
        p.useCats = 1

    def _nothing(self, *args):                 # the default of the hooks a mode may leave alone
        return {}
    check_params = accumulate = summarize = derive = derive_category = set_pass_params = _nothing

    def up(self, up):                          # the ground plane of mode BEV
        return tuple(float(v) for v in (BEV_UP if up is None else up))

    def similarity(self, ev, b_d, b_g, dt_sizes, gt_sizes, pairs):
        t1, t2 = _pair_index(pairs, b_d.device)
        return _xywh_iou(b_d[t1], b_g[t2]), {}

    def line(self, name, short, thr, area, max_dets, value):
        return "mode={} ".format(self.name) + self.fmt.format(name, short, thr, area, max_dets, value)

    def single_class(self, res, name):         # _derive_results skips the per-category part for a single class
        res["AP-" + name] = res["AP"]


class Mode3D(Mode2D):
    """the 3D protocol: IoU3D of the `bbox3D` corners, `ignore3D`, depth ranges"""
    name = "3D"
    ignore_key, box_key, range_key, box_shape = "ignore3D", "bbox3D", "depth", (-1, 8, 3)
    iou_range, area_rng, area_lbl = (0.05, 0.5), [[0, 1e5], [0, 10], [10, 35], [35, 1e5]], ["all", "near", "medium", "far"]
    thresholds = [0.15, 0.25, 0.50]
    fmt = " {:<18} {} @[ IoU={:<9} | depth={:>6s} | maxDets={:>3d} ] = {:0.3f}"
    metrics = ["AP", "AP15", "AP25", "AP50", "APn", "APm", "APf"]
    error_thrs, loc_errors = (0.25, 0.05), True           # the middle and the bottom of the AP3D threshold range

    def groups(self, E, ev, b_d, b_g, dt_sizes, gt_sizes, pairs):
        return E.box3d_overlap_groups(b_d, b_g, dt_sizes, gt_sizes, pairs=pairs)

    def similarity(self, ev, b_d, b_g, dt_sizes, gt_sizes, pairs):
        from . import omni3d_evaluation as E   # the pair passes are looked up where callers (and tests) find them
        mats = self.groups(E, ev, b_d, b_g, dt_sizes, gt_sizes, pairs)
        return (torch.cat([m.reshape(-1) for m in mats]) if mats else torch.zeros(0, device=b_d.device)), {}


class ModeBEV(Mode3D):
    """the 3D protocol (thresholds, depth ranges), so AP-BEV compares with AP3D, on the IoU of the footprints"""
    name = "BEV"
    switch, extension, results, concat_ci = "eval_bev", True, "results_bev", False

    def groups(self, E, ev, b_d, b_g, dt_sizes, gt_sizes, pairs):
        return E.bev_overlap_groups(b_d, b_g, dt_sizes, gt_sizes, up=ev.up, pairs=pairs)

    def row(self, iters, r, categories):
        """the row of `results_bev`: APBEV = mean of the per-category APs like AP3D, then the headline columns"""
        return {"iters": iters, **_ap_columns("APBEV", r, categories, self.metrics)}


def _dist_up(up):
    """None, or the unit vector along three finite numbers (ValueError otherwise)"""
    return None if up is None else tperr.unit_up(up)


def _dist_params(params):
    """None or a dict with some of distThrs / tpDist / minRecall -> a checked copy"""
    if params is None:
        return {}
    if not isinstance(params, dict) or set(params) - {"distThrs", "tpDist", "minRecall"}:
        raise ValueError("dist_params must be a dict with keys out of %r" % (("distThrs", "tpDist", "minRecall"),))
    out = dict(params)
    if "distThrs" in out:
        out["distThrs"] = [float(v) for v in out["distThrs"]]
    thrs = out.get("distThrs", ModeDIST.dist_thrs)
    if float(out.get("tpDist", ModeDIST.tp_dist)) not in thrs:
        raise ValueError("tpDist must be one of distThrs")
    return out


class ModeDIST(Mode3D):
    """the 3D protocol's depth ranges and maxDets; a match needs dist <= d for d in distThrs (metres).  iouThrs holds the
    thresholds mapped to the similarity 1 / (1 + dist) the matching kernel compares (`Omni3Deval.evaluate` refreshes it from
    distThrs); the TP errors are taken at tpDist along the recall thresholds >= minRecall"""
    name = "DIST"
    dist_thrs, tp_dist, min_recall = [0.5, 1.0, 2.0, 4.0], 2.0, 0.1
    thresholds, shown = [0.5, 1.0, 2.0], "distThrs"       # thresholds are named, and looked up, in metres
    fmt = " {:<18} {} @[ dist={:<9}| depth={:>6s} | maxDets={:>3d} ] = {:0.3f}"
    metrics = ["AP", "AP@0.5m", "AP@1m", "AP@2m", "APn", "APm", "APf"]
    switch, up_option, extension, results, concat_ci = "eval_dist", "dist_up", True, "results_dist", False
    options = {"dist_up": _dist_up, "dist_params": _dist_params}
    error_thrs, loc_errors = None, False                  # matched by distance: no background overlap, no error analysis

    def set_params(self, p):
        Mode3D.set_params(self, p)
        p.distThrs, p.tpDist, p.minRecall = np.array(self.dist_thrs), self.tp_dist, self.min_recall
        p.iouThrs = 1.0 / (1.0 + p.distThrs)

    def check_params(self, p):
        p.distThrs = np.asarray(p.distThrs, dtype=np.float64).reshape(-1)
        if not (np.isfinite(p.distThrs).all() and (p.distThrs >= 0).all()):
            raise ValueError("distThrs must be finite and >= 0")
        if not np.any(p.distThrs == float(p.tpDist)):
            raise ValueError("tpDist %r is not one of distThrs %r" % (p.tpDist, p.distThrs.tolist()))
        if not 0.0 <= float(p.minRecall) <= 1.0:
            raise ValueError("minRecall must lie in [0, 1]")
        p.iouThrs = 1.0 / (1.0 + p.distThrs)

    up = staticmethod(_dist_up)                # None: the full 3D distance

    def similarity(self, ev, b_d, b_g, dt_sizes, gt_sizes, pairs):
        from . import omni3d_evaluation as E
        pair_err, _ = E.dist_errors_groups(b_d, b_g, dt_sizes, gt_sizes, up=ev.up, warn=True, pairs=pairs)
        return (1.0 / (1.0 + pair_err[:, 0])).float(), {"pair_err": pair_err}                 # in double; +inf -> 0

    def accumulate(self, ev, pe, t, tod):
        # the lists were cut to the largest maxDets in evaluate(): every detection takes part
        ti = int(np.flatnonzero(np.asarray(pe.distThrs) == float(pe.tpDist))[0])
        tp_err, tp_cnt = tperr.tp_errors(t["order"], t["cat_off"], t["dt_match"][:, ti].contiguous(), t["dt_ignore"][:, ti].contiguous(),
                                         tod(t["pair_row"]), ev._dev["pair_err"], t["npig"], t["has_e"], t["rec_thrs"], float(pe.minRecall))
        return {"tp_errors": tp_err.cpu().numpy(), "tp_count": tp_cnt.cpu().numpy()}

    def summarize(self, ev, one, lines):
        p = ev.params
        aall = p.areaRngLbl.index("all")
        ev.tp_stats = np.full((3,), -1.0)
        for j, (name, short) in enumerate((("Translation Error", "(mATE)"), ("Scale Error", "(mASE)"), ("Orientation Error", "(mAOE)"))):
            v = ev.eval["tp_errors"][:, aall, j]
            ev.tp_stats[j] = np.mean(v[v > -1]) if (v > -1).any() else -1.0
            lines.append(self.line(name, short, "{:0.2f}".format(float(p.tpDist)), "all", p.maxDets[-1], ev.tp_stats[j]))

    def derive(self, ev):
        return {"m" + n: float(ev.tp_stats[j] if ev.tp_stats[j] > -1 else "nan") for j, n in enumerate(_TP_NAMES)}

    def derive_category(self, ev, k, name):
        tp = ev.eval["tp_errors"][k, 0]
        return {n + "-" + name: float(tp[j] if tp[j] > -1 else "nan") for j, n in enumerate(_TP_NAMES)}

    def single_class(self, res, name):
        Mode3D.single_class(self, res, name)
        res.update({n + "-" + name: res["m" + n] for n in _TP_NAMES})

    def set_pass_params(self, p, opts):
        for key, value in opts["dist_params"].items():
            setattr(p, key, np.asarray(value, dtype=np.float64) if key == "distThrs" else float(value))

    def row(self, iters, r, categories):
        """the row of `results_dist`: APDIST = mean of the per-category APs like AP3D, the headline columns, the three mean errors"""
        return {"iters": iters, **_ap_columns("APDIST", r, categories, self.metrics), **{"m" + n: r["m" + n] for n in _TP_NAMES}}


def _let_params(params):
    """None or a dict with some of lonTolFrac / lonTolMin -> a checked copy"""
    if params is None:
        return {}
    if not isinstance(params, dict) or set(params) - {"lonTolFrac", "lonTolMin"}:
        raise ValueError("let_params must be a dict with keys out of %r" % (("lonTolFrac", "lonTolMin"),))
    frac, tmin = let.check_tolerance(params.get("lonTolFrac", let.TOL_FRAC), params.get("lonTolMin", let.TOL_MIN))
    return {k: v for k, v in (("lonTolFrac", frac), ("lonTolMin", tmin)) if k in params}


class ModeLET(Mode3D):
    """the 3D protocol (thresholds on the longitudinal-error-tolerant IoU3D, depth ranges, maxDets); a detection may slide along
    its line of sight by up to max(lonTolFrac x range of the ground truth, lonTolMin metres)"""
    name = "LET"
    switch, extension, results, concat_ci = "eval_let", True, "results_let", False
    options = {"let_params": _let_params}

    def set_params(self, p):
        Mode3D.set_params(self, p)
        p.lonTolFrac, p.lonTolMin = let.TOL_FRAC, let.TOL_MIN

    def check_params(self, p):
        try:
            p.lonTolFrac, p.lonTolMin = let.check_tolerance(p.lonTolFrac, p.lonTolMin)
        except ValueError:
            raise ValueError("lonTolFrac must be finite and >= 0, lonTolMin finite and > 0") from None

    def similarity(self, ev, b_d, b_g, dt_sizes, gt_sizes, pairs):
        from . import omni3d_evaluation as E
        p = ev.params
        flat, pair_aff, pair_lon, _ = E.let_overlap_groups(b_d, b_g, dt_sizes, gt_sizes, p.lonTolFrac, p.lonTolMin, warn=True, pairs=pairs)
        return flat, {"pair_aff": pair_aff, "pair_lon": pair_lon}

    def accumulate(self, ev, pe, t, tod):
        prec_l, tp_aff, tp_lon = let.accumulate_let(t["order"], t["cat_off"], t["rank"], t["dt_match"], t["dt_ignore"], tod(t["pair_row"]),
                                                    ev._dev["pair_aff"], ev._dev["pair_lon"], t["npig"], t["has_e"], t["rec_thrs"], t["max_dets"])
        return {"precision_l": prec_l.cpu().numpy(), "tp_affinity": tp_aff.cpu().numpy(), "tp_lon": tp_lon.cpu().numpy()}

    def summarize(self, ev, one, lines):
        p, L, md, title = ev.params, ev.params.areaRngLbl, ev.params.maxDets, ("Longitudinal Prec.", "(APL)")
        ev.stats_l = np.array([one(1, iouThr=t, areaRng=a, maxDets=m, table="precision_l", title=title)        # the seven AP slots
                               for _, t, a, m in _stat_slots(p, self.name)[:7]], dtype=np.float64)
        aall, ti = L.index("all"), np.where(np.isclose(_LET_TP_IOU, np.asarray(p.iouThrs).astype(float)))[0]
        ev.let_stats = np.full((2,), -1.0)
        for j, (name, short, key) in enumerate((("Long. Affinity", "(mAFF)", "tp_affinity"), ("Long. Error [m]", "(mLON)", "tp_lon"))):
            if len(ti):                                             # tp_lon is signed: the affinity says where there is a value
                has = ev.eval["tp_affinity"][ti[0], :, aall, -1] > -1
                if has.any():
                    ev.let_stats[j] = np.mean(ev.eval[key][ti[0], :, aall, -1][has])
            lines.append(self.line(name, short, "{:0.2f}".format(_LET_TP_IOU), "all", md[-1], ev.let_stats[j]))

    def derive(self, ev):                      # the same seven slots on the longitudinal precision, and the two diagnostics (not x100)
        res = {name.replace("AP", "APL", 1): _percent(ev.stats_l[i]) for i, name in enumerate(self.metrics)}
        res["mAFF"] = float(ev.let_stats[0] if ev.let_stats[0] > -1 else "nan")
        res["mLON"] = float(ev.let_stats[1] if ev.let_stats[0] > -1 else "nan")
        return res

    def derive_category(self, ev, k, name):
        return {"APL-" + name: _table_ap(ev.eval["precision_l"], k)}

    def single_class(self, res, name):
        Mode3D.single_class(self, res, name)
        res["APL-" + name] = res["APL"]

    def set_pass_params(self, p, opts):
        for key, value in opts["let_params"].items():
            setattr(p, key, float(value))

    def row(self, iters, r, categories):
        """the row of `results_let`: APLET / APLLET = means of the per-category LET-AP / LET-APL like AP3D, the headline columns of
        both, the mean affinity and the mean signed longitudinal error (metres) of the true positives"""
        return {"iters": iters, **_ap_columns("APLET", r, categories, self.metrics), **_ap_columns("APLLET", r, categories, self.metrics, "APL"),
                "mAFF": r["mAFF"], "mLON": r["mLON"]}


MODES = {M.name: M() for M in (Mode2D, Mode3D, ModeBEV, ModeDIST, ModeLET)}
_METRICS = {name: M.metrics for name, M in MODES.items()}


# the headline slots of summarize(), shared with the bootstrap
def _stat_slots(p, mode):
    """the 13 `stats` of summarize() as (ap, iouThr, areaRng label, maxDets): AP overall, at three thresholds, in three ranges; AR at
    the three maxDets and in three ranges"""
    thres, L, md = MODES[mode].thresholds, p.areaRngLbl, p.maxDets
    return [(1, None, "all", 100)] + [(1, thres[i], "all", md[2]) for i in range(3)] + [(1, None, L[1 + i], md[2]) for i in range(3)] \
        + [(0, None, "all", md[i]) for i in range(3)] + [(0, None, L[1 + i], md[2]) for i in range(3)]


def _slot_indices(p, mode, ap, iouThr, areaRng, maxDets):
    """-> (indices of the thresholds or None = all, of the ranges, of the maxDets) one slot of summarize() averages over"""
    shown = getattr(p, MODES[mode].shown)
    aind = [i for i, a in enumerate(p.areaRngLbl) if a == areaRng]
    mind = [i for i, m in enumerate(p.maxDets) if m == maxDets]
    tind = None
    if iouThr is not None:
        tind = np.where(np.isclose(iouThr, np.asarray(shown).astype(float)))[0] if ap == 1 else np.where(iouThr == np.asarray(shown))[0]
    return tind, aind, mind


def enabled_modes(only_2d, **switches):
    """The one place that maps the drivers' public switches (eval_bev, eval_dist, eval_let) to the modes of a run: 2D, 3D unless
    only_2d, and -- extensions the reference does not have, off by default -- BEV, DIST and LET after them"""
    return [name for name, M in MODES.items() if name == "2D" or not only_2d and (M.switch is None or switches[M.switch])]


def check_options(**kw):
    """the drivers' other keywords (bev_up, dist_up, dist_params, let_params), checked in the order given -> the options of a pass"""
    checks = {key: check for M in MODES.values() for key, check in M.options.items()}
    return {key: checks[key](value) for key, value in kw.items()}
