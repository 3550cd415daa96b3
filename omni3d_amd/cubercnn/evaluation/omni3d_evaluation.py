"""The evaluator (reference cubercnn/evaluation/omni3d_evaluation.py) and the import surface of this package.  `Omni3Deval` runs the
COCO-style greedy matching and the precision / recall accumulation on the device, around one pair pass over all (image, category)
groups (pairs.py: `box3d_overlap`, `box3d_overlap_groups` and their kin, `evaluate_groups`); what differs by mode is in the mode table
(modes.py), the bootstrap statistics in bootstrap_stats.py, and `Omni3DEvaluator` / `Omni3DEvaluationHelper`, the per-split drivers
`tools/train_net.py:do_test` uses, in drivers.py.  Every public name of those files is importable from here.

Extension without a counterpart in the reference: mode "BEV" = the 3D protocol with the IoU of the cuboids' footprints on the ground
plane (`bev_overlap_groups`, csrc/bev_iou.hip) in place of IoU3D, i.e. the AP-BEV of the outdoor benchmarks; `eval_bev` switches it
on in the two drivers, off by default.

A second one: mode "DIST" = the centre-distance protocol of nuScenes (`dist_errors_groups`, csrc/tp_errors.hip): detections are matched
by the distance of the fitted centres, and the matched pairs are scored for translation, scale and orientation error along the recall
curve (ATE / ASE / AOE); `eval_dist` switches it on in the two drivers, off by default.  See `Omni3Deval`.

A third one: mode "LET" = the longitudinal-error-tolerant metrics of the Waymo camera-only benchmark (`let_overlap_groups`,
csrc/let_iou.hip): a detection may slide along its own line of sight onto the ground truth within a tolerance that grows with range, the
exact IoU3D of the slid box decides the match (LET-AP), and a second table scales precision by how little sliding was needed (LET-APL);
`eval_let` switches it on in the two drivers, off by default.  See `Omni3Deval`.

A fourth one, for every mode: `Omni3Deval.bootstrap` / `bootstrap_compare` = image-level bootstrap confidence intervals of AP / AR and
the paired comparison of two prediction sets.  The match tables of evaluate() are kept and all replicates are accumulated in one launch
from integer image multiplicities (`kernels.bootstrap`, csrc/eval_bootstrap.hip); `bootstrap` switches it on in the two drivers, off by
default.  See `Omni3Deval.bootstrap`.

A fifth one, for every mode but DIST: `Omni3Deval.errors` / `summarize_errors` = the error decomposition after TIDE: every false positive
is typed (wrong class, poor box, both, duplicate, background), every unfound ground truth is a miss, and each type is priced by the AP an
oracle repairing it alone would gain (error_types.py, `kernels.errtypes`, csrc/eval_errors.hip); `errors` switches it on in the two
drivers, off by default.  See `Omni3Deval.errors`.

The reference's `params.useCats = 0` (class-agnostic evaluation: one group per image, K = 1) is built for every mode; its accumulation
over one long list has a kernel of its own (`kernels.accumulate`, csrc/eval_accumulate_par.hip); `eval_agnostic` adds such a pass per mode
in the two drivers, off by default, and `proposal_recall` (proposals.py) scores region proposals with it.  See `Omni3Deval`."""
import copy
import datetime

import numpy as np
import torch

from ...kernels import accumulate as kacc
from ...kernels import iou3d
from .bootstrap_stats import BOOTSTRAP_CHUNK, _bootstrap_result, _check_confidence, bootstrap_compare, bootstrap_weights  # noqa: F401
from .error_types import ERROR_TYPES, ORACLES, error_analysis, error_lines  # noqa: F401
from .modes import _METRICS, MODES, _slot_indices, _stat_slots  # noqa: F401
from .pairs import (BEV_UP, _pair_index, _ragged_pairs, _xywh_iou, bev_overlap_groups, box3d_overlap, box3d_overlap_groups,  # noqa: F401
                    dist_errors_groups, evaluate_groups, let_overlap_groups)


# =====================================================================================================================
# Omni3Deval: evaluate -> accumulate -> summarize on the device (reference :1019-1704)
# =====================================================================================================================
MAX_GROUP_GT = 1024                            # ground truths per group `eval_match_kernel` holds (csrc/eval_match.hip EVAL_MAXG)


class Omni3DParams:
    """omni3d_evaluation.py:1019-1088; the defaults of each mode are its `set_params` in modes.py"""

    def __init__(self, mode="2D"):
        if mode not in MODES:
            raise Exception("mode %s not supported" % (mode))
        MODES[mode].set_params(self)
        self.iouType = "bbox"
        self.mode = mode
        self.proximity_thresh = 0.3


class AnnotationIndex:
    """The four COCO-API calls Omni3Deval makes (getImgIds / getCatIds / getAnnIds / loadAnns) over a plain list of
    annotation dicts -- pycocotools is not needed for the scoped path."""

    def __init__(self, anns, img_ids=None, cat_ids=None):
        self.anns = {}
        for i, a in enumerate(anns):
            a.setdefault("id", i + 1)
            self.anns[a["id"]] = a
        self._imgs = sorted(set(img_ids) if img_ids is not None else {a["image_id"] for a in anns})
        self._cats = sorted(set(cat_ids) if cat_ids is not None else {a["category_id"] for a in anns})

    def getImgIds(self):
        return list(self._imgs)

    def getCatIds(self):
        return list(self._cats)

    def getAnnIds(self, imgIds=(), catIds=()):
        imgs, cats = set(imgIds), set(catIds)
        return [i for i, a in self.anns.items() if (not imgs or a["image_id"] in imgs) and (not cats or a["category_id"] in cats)]

    def loadAnns(self, ids):
        return [self.anns[i] for i in ids]


class Omni3Deval:
    """`Omni3Deval(cocoGt, cocoDt, mode=...)` with the reference's evaluate() / accumulate() / summarize() and result layout
    (`eval['precision']` [T,R,K,A,M], `eval['recall']` [T,K,A,M], `eval['scores']`, `stats` (13,)).

    evaluate(): all (image, category) groups at once -- one IoU pass (`box3d_overlap_groups` in 3D, `bev_overlap_groups` with the
    up vector `up` in BEV -- which otherwise is the 3D mode: `bbox3D`, `ignore3D`, `depth` --, a vectorised box IoU in 2D) and one greedy-matching launch for every group x range x threshold (`evaluate_groups`, csrc/eval_match.hip);
    accumulate(): one launch for every (category, range, maxDets, threshold) (`omni_eval_accumulate`).  The reference runs
    these as Python loops over dict-of-list structures (:1339-1351, :1230-1301).

    eval_prox (proximity evaluation for non-exhaustively annotated datasets, :1419-1429, :1499, :1534-1536): a detection may
    only match ground truths whose 2D box overlaps its own by more than `params.proximity_thresh`, and a detection with no
    ground truth in proximity is ignored.  True / False like the reference, or a collection of image ids (extension: the
    helper evaluates the union of several datasets of which only some use proximity evaluation).

    `params.useCats = 0` (class-agnostic evaluation, the reference's switch :1147-1153, :1188-1203, :1328-1336, :1368-1374, :1441-1447;
    every mode): all records of `imgIds` are loaded whatever `catIds` says; there is ONE group per image, its ground truths and its
    detections gathered category-major in the order of `params.catIds` (not made unique; records of a category that is not in it take
    no part) and then in record order, the detections stably sorted by descending score and cut to `maxDets[-1]`; matching, ignore
    rules, ranges and eval_prox apply to those groups unchanged, and K = 1 in every table (`tp_errors`, `precision_l`, ... and
    `bootstrap()` included).  An image with more than 1024 ground truths raises ValueError before any launch (the matching kernel holds
    that many per group); `errors()` raises ValueError.  Departure from the reference: its accumulate() overwrites `params.catIds` with
    [-1], after which its own evaluate() cannot run again; here `params.catIds` stays what the user set and `evalImgs` reports
    `category_id` -1.  accumulate() then takes `omni_eval_accumulate_par` (csrc/eval_accumulate_par.hip: the one list of all detections
    cut into blocks over many workgroups, the same bits) from `kernels.accumulate.PAR_MIN_LIST` detections on.

    Mode "DIST" (extension, the centre-distance protocol of nuScenes; `up` = None or the up vector of the ground plane).
    Boxes: both sides are the eight `bbox3D` corners in the order of `boxgen.UNIT`, fitted by `cuboid_fit` (default eps_dim, fit_tol);
    an invalid box on either side has distance +inf and matches nothing.
    Distance: the Euclidean distance of the fitted centres; with `up`, the distance in the ground plane orthogonal to it (nuScenes'
    definition; (0, -1, 0) for level outdoor cameras).  The default is the full 3D distance: Omni3D has no world frame and indoor
    cameras are pitched.
    Matching: the 3D protocol (depth ranges, `ignore3D`, maxDets, eval_prox; `evaluate_groups` unchanged) on the similarity
    s = 1 / (1 + dist), computed in double and stored as float32 (0 for +inf), against the thresholds 1 / (1 + d), d in
    `params.distThrs` (default 0.5, 1, 2, 4 m); `params.iouThrs` holds the mapped thresholds.  Departures from nuScenes: a match needs
    dist <= d (nuScenes: <), and AP is this evaluator's 101-point AP averaged over the distance thresholds, without nuScenes' 10 %
    recall and precision clipping.
    TP metrics: at `params.tpDist` (default 2.0, one of distThrs) and the largest maxDets, per category and depth range: the
    category's detections in the merge order of accumulate(), the ignored ones skipped; at the c-th true positive m_c = the mean of
    (trans, scale, orient) of `kernels.tperr` over the first c; the recall threshold r_j of `params.recThrs` takes m_c when r_j >=
    `params.minRecall` (default 0.1) and (c-1)/npig < r_j <= c/npig; the metric is the mean of the values taken, -1 without ground
    truth or evaluated image, 1.0 when no threshold took a value (nuScenes' rule).  Departure: nuScenes interpolates over confidence,
    this is the step rule above.  accumulate() fills `eval['tp_errors']` (K, A, 3) and `eval['tp_count']` (K, A); summarize() keeps
    the `stats` layout (slots 1..3: AP at 0.5, 1 and 2 m, looked up in distThrs), appends mATE / mASE / mAOE = the means over the
    categories with a value > -1 at range "all", and sets `tp_stats`.  No composite score: NDS needs velocity and attribute errors
    one image does not give.

    Mode "LET" (extension, LET-3D-AP / LET-3D-APL of Hung et al. 2022, the Waymo camera-only metric: is the detector wrong, or only
    wrong in depth?).  Boxes as in mode "DIST": the eight `bbox3D` corners in the order of `boxgen.UNIT`, in camera coordinates, both
    sides fitted by `cuboid_fit`; the sensor origin is the camera centre.
    Pair: for a detection with fitted centre P and a ground truth with fitted centre G, u = P / |P| is the line of sight, lon =
    (G - P) . u the signed longitudinal error (positive: predicted too near), T = max(lonTolFrac |G|, lonTolMin) (defaults 0.10 and
    0.5 m, Waymo's values), aff = 1 - min(|lon| / T, 1) the longitudinal affinity; the aligned box is the detection with its centre
    moved to P + lon u, the point of its ray closest to G; let_iou = the exact cuboid IoU3D (csrc/cuboid_exact.h, in double, stored
    as float32) of the aligned box and the ground truth when aff > 0, exactly 0 when aff == 0.  An invalid box on either side or a
    detection on the sensor (|P| <= 1e-8) gives (0, 0, NaN) and matches nothing.
    Matching: the 3D protocol (iouThrs 0.05 .. 0.5, depth ranges, `ignore3D`, maxDets, eval_prox; `evaluate_groups` unchanged) on
    let_iou; LET-AP is this evaluator's 101-point AP on those matches (`eval['precision']`, `stats`).  Departures from Waymo: Waymo
    matches bipartitely on the longitudinal affinity, this is the greedy COCO matching by descending score on let_iou;
    Waymo thresholds at one IoU per class and bins by difficulty level, here the ten IoU thresholds and the depth ranges of AP3D
    apply; the exact IoU3D decides, not the pair algorithm AP3D keeps for comparability (a slid box is a near-aligned near-duplicate,
    where that algorithm is off by up to 0.3).
    LET-APL: on the same lists and recall axis the precision at a list position is (sum of aff over the true positives so far) /
    (tp + fp + eps), aff of the pair (detection, its matched ground truth); made monotone from the right and sampled at recThrs like
    precision: `eval['precision_l']` (T, R, K, A, M), -1 where precision is, never above precision.  `eval['tp_affinity']` and
    `eval['tp_lon']` (T, K, A, M): the mean aff and the mean signed lon (metres; its sign tells whether a category is predicted
    systematically near or far) of the true positives among the included detections, -1 without one.  summarize() keeps the `stats`
    layout, sets `stats_l` (7,) = LET-APL overall, at 0.15 / 0.25 / 0.50, near / medium / far, and `let_stats` (2,) = mean affinity
    and mean signed longitudinal error at range "all", the largest maxDets and IoU 0.25, as means over the categories with a true
    positive (-1 without any), and prints those lines too."""

    def __init__(self, cocoGt=None, cocoDt=None, iouType="bbox", mode="2D", eval_prox=False, up=None):
        if mode not in MODES:
            raise Exception("mode %s not supported" % (mode))
        self.mode, self.eval_prox, self._mode = mode, eval_prox, MODES[mode]
        self.up = self._mode.up(up)
        self.cocoGt, self.cocoDt = cocoGt, cocoDt
        self.params = Omni3DParams(mode)
        self.eval, self.stats, self._dev = {}, [], None
        if cocoGt is not None:
            self.params.imgIds = sorted(cocoGt.getImgIds())
            self.params.catIds = sorted(cocoGt.getCatIds())

    # ---- evaluate (:1315-1357 + computeIoU :1359-1431 + evaluateImg :1433-1551) ----------------------------------------
    def evaluate(self, device=None):
        p = self.params
        p.imgIds = list(np.unique(p.imgIds))
        p.catIds = list(np.unique(p.catIds)) if p.useCats else p.catIds
        p.maxDets = sorted(p.maxDets)
        load = {"catIds": p.catIds} if p.useCats else {}      # useCats = 0: all records of the images, whatever catIds says (:1151-1153)
        gts = self.cocoGt.loadAnns(self.cocoGt.getAnnIds(imgIds=p.imgIds, **load))
        dts = self.cocoDt.loadAnns(self.cocoDt.getAnnIds(imgIds=p.imgIds, **load))
        M = self._mode
        flag, key, rng_key = M.ignore_key, M.box_key, M.range_key
        g_by, d_by = {}, {}
        for g in gts:
            g[flag] = g[flag] if flag in g else 0
            g_by.setdefault((g["image_id"], g["category_id"]), []).append(g)
        for d in dts:
            d_by.setdefault((d["image_id"], d["category_id"]), []).append(d)
        M.check_params(p)
        maxDet = p.maxDets[-1]
        # group table in (category, image) order = the order evalImgs / accumulate walk (:1346-1351, :1230-1241)
        groups = []
        for ki, cat in enumerate(p.catIds if p.useCats else [-1]):
            for ii, img in enumerate(p.imgIds):
                if p.useCats:
                    g, d = g_by.get((img, cat), []), d_by.get((img, cat), [])
                else:                                          # one group per image: category-major in catIds order, then record order (:1373-1374)
                    g = [x for c in p.catIds for x in g_by.get((img, c), [])]
                    d = [x for c in p.catIds for x in d_by.get((img, c), [])]
                    if len(g) > MAX_GROUP_GT:
                        raise ValueError("image %s has %d ground truths; the matching kernel holds %d per group" % (img, len(g), MAX_GROUP_GT))
                if not g and not d:
                    continue
                order = np.argsort([-x["score"] for x in d], kind="mergesort")
                groups.append((ki, ii, g, [d[i] for i in order[:maxDet]]))
        dt_sizes = np.array([len(gr[3]) for gr in groups], dtype=np.int64)
        gt_sizes = np.array([len(gr[2]) for gr in groups], dtype=np.int64)
        all_d = [x for gr in groups for x in gr[3]]
        all_g = [x for gr in groups for x in gr[2]]
        if device is None:
            device = torch.device("cpu") if iou3d._lib.get().emulated else torch.device("cuda")
        f32 = lambda v, shape: torch.tensor(np.asarray(v, dtype=np.float32).reshape(shape)).to(device)      # noqa: E731
        pairs = _ragged_pairs(dt_sizes, gt_sizes)              # built once: the similarity pass and the proximity rule share it
        flat, extra = M.similarity(self, f32([x[key] for x in all_d], M.box_shape), f32([x[key] for x in all_g], M.box_shape), dt_sizes, gt_sizes, pairs)
        far = None
        if self.eval_prox is not False and self.eval_prox is not None and len(all_d) and len(all_g):
            t1, t2 = _pair_index(pairs, device)
            # the similarity of a mode that matches on `bbox` is this 2D IoU already
            iou2d = flat if key == "bbox" else _xywh_iou(f32([x["bbox"] for x in all_d], (-1, 4))[t1], f32([x["bbox"] for x in all_g], (-1, 4))[t2])
            prox = iou2d > p.proximity_thresh
            if self.eval_prox is not True:            # only the images named
                chosen = set(self.eval_prox)
                applies = np.repeat(np.array([p.imgIds[gr[1]] in chosen for gr in groups], dtype=bool), dt_sizes)
                t_app = torch.from_numpy(applies).to(device)
                prox = prox | ~t_app[t1]
            else:
                t_app = torch.ones(len(all_d), dtype=torch.bool, device=device)
            flat = torch.where(prox, flat, torch.full_like(flat, -1.0))      # a pair out of proximity can never be a match
            near = torch.zeros(len(all_d), dtype=torch.int32, device=device).index_add_(0, t1, prox.to(torch.int32)) > 0
            has_gt = torch.from_numpy(np.repeat(gt_sizes > 0, dt_sizes)).to(device)
            far = ~near & has_gt & t_app
        m = evaluate_groups(flat, dt_sizes, gt_sizes, torch.tensor([int(x[flag]) for x in all_g], dtype=torch.int32, device=device),
                            f32([x[rng_key] for x in all_g], (-1,)), f32([x[rng_key] for x in all_d], (-1,)), p.areaRng, p.iouThrs)
        if far is not None:
            m["dt_ignore"] = (m["dt_ignore"].bool() | far.view(1, 1, -1)).to(m["dt_ignore"].dtype)
        self._dev = {"groups": groups, "dt_sizes": dt_sizes, "gt_sizes": gt_sizes, "match": m, "device": device,
                     "scores": np.array([x["score"] for x in all_d], dtype=np.float64),
                     "dt_ids": np.array([x.get("id", 0) for x in all_d]), "gt_ids": np.array([x.get("id", 0) for x in all_g])}
        self._dev.update(extra)
        self._paramsEval = copy.deepcopy(self.params)
        self._evalImgs = None

    @property
    def evalImgs(self):
        """the reference's per-(category, range, image) list of dicts (:1541-1551), materialised on demand from the device
        results -- accumulate() does not need it"""
        if self._evalImgs is None and self._dev is not None:
            p, d = self._paramsEval, self._dev
            m = {k: v.cpu().numpy() for k, v in d["match"].items()}
            doff, goff = np.concatenate([[0], np.cumsum(d["dt_sizes"])]), np.concatenate([[0], np.cumsum(d["gt_sizes"])])
            where = {(ki, ii): n for n, (ki, ii, _, _) in enumerate(d["groups"])}
            out = []
            for ki, cat in enumerate(p.catIds if p.useCats else [-1]):
                for ai, aRng in enumerate(p.areaRng):
                    for ii, img in enumerate(p.imgIds):
                        n = where.get((ki, ii))
                        if n is None:
                            out.append(None)
                            continue
                        ds, gs = slice(doff[n], doff[n + 1]), slice(goff[n], goff[n + 1])
                        order = m["gt_order"][ai, gs]
                        gids, dids = d["gt_ids"][gs], d["dt_ids"][ds]
                        dtm = m["dt_match"][ai][:, ds]
                        gtm = m["gt_match"][ai][:, gs][:, order]
                        out.append({"image_id": img, "category_id": cat, "aRng": aRng, "maxDet": p.maxDets[-1],
                                    "dtIds": list(dids), "gtIds": list(gids[order]),
                                    "dtMatches": np.where(dtm >= 0, gids[np.clip(dtm, 0, None)] if len(gids) else 0, 0).astype(np.float64),
                                    "gtMatches": np.where(gtm >= 0, dids[np.clip(gtm, 0, None)] if len(dids) else 0, 0).astype(np.float64),
                                    "dtScores": list(d["scores"][ds]), "gtIgnore": m["gt_ignore"][ai, gs][order].astype(np.float64),
                                    "dtIgnore": m["dt_ignore"][ai][:, ds].astype(bool)})
            self._evalImgs = out
        return self._evalImgs

    def _merge_tables(self, K, A):
        """the host tables accumulate() and bootstrap() hand to the device: the merge order, the rank of a detection in its image's
        list, the row of its first pair in the flat pair tensors of evaluate(), the ground-truth counts; per (image, category) group
        its category, image index and non-ignored ground truths per range"""
        d = self._dev
        groups, dt_sizes, gt_sizes = d["groups"], d["dt_sizes"], d["gt_sizes"]
        sumD = int(dt_sizes.sum())
        cat_of_group = np.array([g[0] for g in groups], dtype=np.int64)
        det_cat = np.repeat(cat_of_group, dt_sizes)
        det_rank = (np.arange(sumD) - np.repeat(np.cumsum(dt_sizes) - dt_sizes, dt_sizes)).astype(np.int32)
        # merge order: stable by -score inside a category, categories ascending; ties keep (image, in-image) order (:1250-1253)
        order = np.lexsort((np.arange(sumD), -d["scores"], det_cat)).astype(np.int32) if sumD else np.zeros(0, np.int32)
        cat_off = np.concatenate([[0], np.cumsum(np.bincount(det_cat, minlength=K))]).astype(np.int32)
        gt_ig = d["match"]["gt_ignore"].cpu().numpy()                                   # (A, sumG)
        gcat = np.repeat(cat_of_group, gt_sizes)
        npig = np.zeros((K, A), np.int32)
        for a in range(A):
            npig[:, a] = np.bincount(gcat[gt_ig[a] == 0], minlength=K)
        has_e = np.bincount(cat_of_group, minlength=K).astype(np.int32).clip(max=1)
        n_gt = np.repeat(gt_sizes, dt_sizes)                  # a detection owns one pair per ground truth of its group, in list order
        pair_row = np.cumsum(n_gt) - n_gt
        return {"cat_of_group": cat_of_group, "det_rank": det_rank, "order": order, "cat_off": cat_off, "gt_ig": gt_ig, "npig": npig,
                "has_e": has_e, "pair_row": pair_row}

    def _device_tables(self, p, tb, tod):
        """what the accumulation kernels of accumulate(), the modes and bootstrap() share, on the device (`pair_row` stays on the host)"""
        m = self._dev["match"]
        return {"order": tod(tb["order"]), "cat_off": tod(tb["cat_off"]), "rank": tod(tb["det_rank"]), "npig": tod(tb["npig"]),
                "has_e": tod(tb["has_e"]), "rec_thrs": tod(np.asarray(p.recThrs, dtype=np.float64)), "max_dets": tod(np.asarray(p.maxDets, dtype=np.int32)),
                "dt_match": m["dt_match"].contiguous(), "dt_ignore": m["dt_ignore"].contiguous(), "pair_row": tb["pair_row"]}

    @staticmethod
    def _num_cats(p):
        return len(p.catIds) if p.useCats else 1

    def _check_same_params(self, p, what):
        pe = self._paramsEval
        if list(p.catIds) != list(pe.catIds) or bool(p.useCats) != bool(pe.useCats) or list(map(tuple, p.areaRng)) != list(map(tuple, pe.areaRng)) or list(p.maxDets) != list(pe.maxDets) \
                or list(p.imgIds) != list(pe.imgIds):
            raise NotImplementedError(what + " with parameters other than evaluate()'s is not built on the device path")

    # ---- accumulate (:1172-1313) --------------------------------------------------------------------------------------
    def accumulate(self, p=None, parallel=None, block=None):
        """parallel / block: which accumulation kernel (`kernels.accumulate.accumulate`); None = `omni_eval_accumulate_par` only under
        useCats = 0 with at least PAR_MIN_LIST detections, else the one-wave kernel.  Both give the same bits."""
        assert self._dev is not None, "Please run evaluate() first"
        if p is None:
            p = self.params
        pe, d = self._paramsEval, self._dev
        self._check_same_params(p, "accumulate()")
        T, R, K, A, M = len(p.iouThrs), len(p.recThrs), self._num_cats(p), len(p.areaRng), len(p.maxDets)
        dev = d["device"]
        sumD = int(d["dt_sizes"].sum())
        tb = self._merge_tables(K, A)
        tod = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)               # noqa: E731
        t = self._device_tables(p, tb, tod)
        t_sc = tod(d["scores"])
        if parallel is None:                                   # the one list of all detections, when it is long enough to pay
            parallel = not p.useCats and sumD >= kacc.PAR_MIN_LIST
        if not parallel:
            prec = torch.full((T, R, K, A, M), -1.0, dtype=torch.float64, device=dev)
            rec = torch.full((T, K, A, M), -1.0, dtype=torch.float64, device=dev)
            scr = torch.full((T, R, K, A, M), -1.0, dtype=torch.float64, device=dev)
            L = iou3d._lib.get()
            _p = iou3d._lib.ptr
            L.call("omni_eval_accumulate", _p(t["order"]), _p(t["cat_off"]), _p(t["rank"]), _p(t_sc), _p(t["dt_match"]), _p(t["dt_ignore"]), _p(t["npig"]),
                   _p(t["has_e"]), _p(t["rec_thrs"]), _p(t["max_dets"]), K, A, M, T, R, sumD, _p(prec), _p(rec), _p(scr), iou3d._lib.stream_of(prec))
        else:
            prec, rec, scr = kacc.accumulate(t["order"], t["cat_off"], t["rank"], t_sc, t["dt_match"], t["dt_ignore"], t["npig"], t["has_e"],
                                             t["rec_thrs"], t["max_dets"], parallel=True, block=block)
        self.eval = {"params": p, "counts": [T, R, K, A, M], "date": datetime.datetime.now().strftime("%Y-%m-%d %H:%M:%S"),
                     "precision": prec.cpu().numpy(), "recall": rec.cpu().numpy(), "scores": scr.cpu().numpy()}
        self.eval.update(self._mode.accumulate(self, pe, t, tod))

    # ---- summarize (:1553-1704) ---------------------------------------------------------------------------------------
    def summarize(self):
        if not self.eval:
            raise Exception("Please run accumulate() first")
        p, ev, mode, M = self.params, self.eval, self.mode, self._mode
        lines = []

        def one(ap=1, iouThr=None, areaRng="all", maxDets=100, table="precision", title=("Average Precision", "(AP)")):
            shown = getattr(p, M.shown)
            iouStr = "{:0.2f}:{:0.2f}".format(shown[0], shown[-1]) if iouThr is None else "{:0.2f}".format(iouThr)
            tind, aind, mind = _slot_indices(p, mode, ap, iouThr, areaRng, maxDets)
            s = ev[table] if ap == 1 else ev["recall"]
            if tind is not None:
                s = s[tind]
            s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
            mean_s = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
            lines.append(M.line(*(title if ap == 1 else ("Average Recall", "(AR)")), iouStr, areaRng, maxDets, mean_s))
            return mean_s

        stats = np.zeros((13,))
        for i, (ap, iouThr, areaRng, maxDets) in enumerate(_stat_slots(p, mode)):
            stats[i] = one(ap, iouThr=iouThr, areaRng=areaRng, maxDets=maxDets)
        self.stats = stats
        M.summarize(self, one, lines)
        return "\n".join(lines)

    def __str__(self):
        self.summarize()

    # ---- bootstrap (extension) ----------------------------------------------------------------------------------------
    def _bootstrap_tables(self, weights, chunk=None):
        """weights (n, I) int32 -> (ap, ar) (n, T, K, A, M) float64 on the host: `kernels.bootstrap` on the tables of evaluate(),
        `chunk` rows of `weights` at a time"""
        from ...kernels import bootstrap as kb
        p, d = self.params, self._dev
        self._check_same_params(p, "bootstrap()")
        chunk = BOOTSTRAP_CHUNK if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError("chunk must be >= 1")
        T, K, A, M = len(p.iouThrs), self._num_cats(p), len(p.areaRng), len(p.maxDets)
        dev, groups, dt_sizes, gt_sizes = d["device"], d["groups"], d["dt_sizes"], d["gt_sizes"]
        tb = self._merge_tables(K, A)
        G = len(groups)
        grp_img = np.array([g[1] for g in groups], dtype=np.int32)
        grp_off = np.concatenate([[0], np.cumsum(np.bincount(tb["cat_of_group"], minlength=K))]).astype(np.int32)
        gid = np.repeat(np.arange(G), gt_sizes)
        grp_npig = np.zeros((G, A), np.int32)
        for a in range(A):
            grp_npig[:, a] = np.bincount(gid[tb["gt_ig"][a] == 0], minlength=G)
        tod = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)               # noqa: E731
        t, t_img = self._device_tables(p, tb, tod), tod(np.repeat(grp_img, dt_sizes).astype(np.int32))
        t_goff, t_gimg, t_gnpig = tod(grp_off), tod(grp_img), tod(grp_npig)
        n = weights.shape[0]
        ap, ar = np.empty((n, T, K, A, M), np.float64), np.empty((n, T, K, A, M), np.float64)
        for c0 in range(0, n, chunk):
            w = tod(weights[c0:c0 + chunk])
            npig_b, has_e_b = kb.bootstrap_counts(t_goff, t_gimg, t_gnpig, w, sum_gt=int(gt_sizes.sum()))
            a1, a2 = kb.bootstrap_accumulate(t["order"], t["cat_off"], t["rank"], t["dt_match"], t["dt_ignore"], t_img, w, npig_b, has_e_b,
                                             t["rec_thrs"], t["max_dets"])
            ap[c0:c0 + chunk], ar[c0:c0 + chunk] = a1.cpu().numpy(), a2.cpu().numpy()
        return ap, ar

    def bootstrap(self, n=1000, seed=0, confidence=0.95, weights=None, strata=None, chunk=None):
        """Image-level bootstrap of the AP / AR this evaluator reports (extension; call after evaluate()): is a difference in AP more
        than the luck of the test set?

        Definition.  A replicate is a vector w of len(params.imgIds) non-negative integers; its result is BY DEFINITION what this
        evaluator returns on the data set in which image i is present w[i] times, each copy with copies of its ground truths and
        detections (w[i] = 0: absent), the copies adjacent in the image order.  evaluate() matches per (image, category) -- per image under useCats = 0 --, so the match
        tables stay; only accumulate() is redone, for all replicates in one launch (`omni_eval_bootstrap`, csrc/eval_bootstrap.hip): in
        the merge order of accumulate() a detection counts as w consecutive identical entries; npig and "has an evaluated image" are the
        weighted sums over the (image, category) groups; precision at the last copy of a true positive is TP / (FP + TP + eps) on the
        weighted inclusive sums, and it serves the recall thresholds in ((TP - w) / npig, TP / npig].  When several detections of a
        category tie in score this weighted order is the definition (a physically duplicated data set would interleave them).
        Scope: `precision` (as its mean over the recall thresholds) and `recall` of all five modes, which share the match tables.  Out
        of scope: the true-positive errors of mode "DIST" and `precision_l` / the affinity tables of mode "LET".

        weights: explicit replicates, (n, I) integers >= 0, columns in the order of params.imgIds (ValueError otherwise).  Without
        them n rows are drawn: g = np.random.default_rng(seed); the strata in sorted label order; a stratum of n_s images fills its
        columns with g.multinomial(n_s, np.full(n_s, 1 / n_s), size=n), so every row sums to I.  strata: None = one stratum, or a
        mapping image id -> label: images are resampled within their label.  chunk: the replicates go to the device `chunk` rows at a
        time (default BOOTSTRAP_CHUNK = 256: the weight table and the two result tables of a chunk take 256 x (4 I + 16 T K A M)
        bytes there); the result does not depend on it, bit for bit.  ValueError when (number of detections or of ground truths) x
        (largest weight) >= 2^31: the weighted counts are 32-bit.

        -> dict: `weights` (n, I) int32; `ap`, `ar` (n, T, K, A, M) float64, -1 where accumulate() leaves -1; `stats` (n, 13) the
        slots of summarize() per replicate (each the mean over the thresholds and categories with a value of `ap` or `ar`); `point`
        (13,) the same from the all-ones replicate = the data set itself; `mean`, `se` (std, ddof=1) and `n_valid` (13,) over the
        replicates whose slot is > -1, `ci` (13, 2) = np.quantile of those at (1 - confidence) / 2 and (1 + confidence) / 2 (NaN
        without a valid replicate, `se` NaN with fewer than two); `per_category`: a dict of the same (`point`, `values` (n, K),
        `mean`, `se`, `n_valid` (K,), `ci` (K, 2)) for the per-category AP at range "all" and the largest maxDets, averaged over the
        thresholds."""
        if self._dev is None:
            raise Exception("Please run evaluate() first")
        confidence = _check_confidence(confidence)
        W = bootstrap_weights(self._paramsEval.imgIds, n, seed, weights, strata)
        ap, ar = self._bootstrap_tables(np.concatenate([np.ones((1, W.shape[1]), np.int32), W]), chunk)      # row 0: the point estimate
        return _bootstrap_result(self.params, self.mode, W, ap, ar, confidence)

    # ---- error decomposition (extension) ------------------------------------------------------------------------------
    def errors(self, t_fg=None, t_bg=None, area="all"):
        """What is the AP lost to?  (Extension, after TIDE: Bolya et al., ECCV 2020; call after evaluate(); modes 2D, 3D, BEV, LET.)
        Every false positive is wrong class, right object but poor box, duplicate or detection on nothing, every unfound ground truth is
        a miss, and each type is priced by the AP gained if an oracle repaired it alone.  Mode DIST raises ValueError: it matches by
        distance, a background overlap has no meaning there.  So does `params.useCats = 0`: without categories there is no wrong class.

        Thresholds.  t_fg must be one of params.iouThrs (np.isclose; ValueError otherwise): the analysis reuses the match tables of
        evaluate() at (area, t_fg, the largest maxDets); 0 < t_bg < t_fg.  Defaults, conventions and not tuned values: 0.5 / 0.1 in 2D
        (TIDE's), 0.25 / 0.05 in 3D / BEV / LET (the middle and the bottom of the AP3D threshold range).  area: one label of
        params.areaRngLbl.
        Image-level similarity.  Per image, rows = all detections that took part in evaluate() (every category's list cut to maxDets),
        category-major in params.catIds order and by descending score inside a category, the order of the group table of evaluate();
        columns = all ground truths of the image in the same category-major order.  One more pass of the mode's own similarity over these
        image groups; the raw similarity also under eval_prox (a detection eval_prox made ignored stays ignored, the proximity mask is not
        applied across categories).
        Candidates: the ground truths that are not `_ignore` at the range.  Types (one code per detection, `kernels.errtypes`): TP =
        matched and not ignored; IGN = ignored; every other detection is a false positive of its category c with s_free / s_used /
        s_other = its largest similarity to an unmatched / a matched candidate of category c / a candidate of another category (-inf for
        an empty set; the later row among equal values, eval_match's rule), and is, in TIDE's precedence, Loc if s_free >= t_bg, else Cls
        if s_other >= t_fg, else Dupe if s_used >= t_fg, else Bkg if all three < t_bg (an image without candidates is all Bkg), else
        Both.  The float32 similarities are compared with the thresholds as doubles.  Attributed ground truth: the arg-max of the
        deciding set for Loc / Cls / Dupe, -1 otherwise.  Miss: an unmatched candidate no Loc or Cls detection is attributed to.
        Departures from TIDE, whose precedence this is: a Loc points to an UNMATCHED candidate of the category only (so its oracle can
        always make it a true positive); a ground truth is spared from Miss by a Loc / Cls attribution only; `>=` / `<` at the thresholds
        are as written here; ignored detections and ground truths follow this evaluator's `_ignore` rules instead of COCO crowds; AP is
        this evaluator's 101-point AP at one threshold and one range, not COCO's mean over thresholds.
        Oracles, each alone on a copy of the tables and followed by an unchanged accumulation (T = A = M = 1): Loc: among the Loc
        detections attributed to one ground truth the highest score wins (the lower row among equal scores) and becomes its true
        positive, the others are removed (set ignored); Cls: the same contest; if the ground truth is matched already all are removed,
        otherwise the winner becomes a true positive IN THE GROUND TRUTH'S CATEGORY (the merge order is rebuilt for it); Both, Dupe, Bkg:
        removed; Miss: npig loses the missed ground truths; FP: every false positive removed; FN: npig = the matched candidates.

        -> dict: `t_fg`, `t_bg`, `area`; `names` = the eight oracles (Cls, Loc, Both, Dupe, Bkg, Miss, FP, FN); in the detection order
        of evaluate() (all detections of category 0 image by image, then category 1, ...): `dt_ids`, `type` (sumD,) int8, `attributed_gt`
        (sumD,) annotation id or -1, `s_free` / `s_used` / `s_other` (sumD,) float32; `missed_gt_ids`; `counts` (K, 6) per category the
        numbers of Cls, Loc, Both, Dupe, Bkg detections and missed ground truths, `counts_total` (6,); `ap` (K,) = the mean of
        precision[t_fg, :, k, area, -1] over the recall thresholds from the unmodified tables (-1 as there); `ap_fixed` (8, K) the same
        under each oracle; `dap` (8, K) = ap_fixed - ap where both are > -1, NaN elsewhere; `dap_mean` (8,) its mean over those
        categories (NaN without one); `dropped` (8,) the categories with an ap that an oracle emptied (Miss / FN: npig 0).  In the
        cuboid modes `loc_errors` (K, 3) = the mean (translation in metres, 1 - aligned IoU, orientation in radians; `kernels.tperr`) over
        the Loc detections of a category and their attributed ground truths -- whether "poor box" means depth, size or rotation --, NaN
        without one, `loc_errors_mean` (3,) over the categories with a value and `loc_skipped` the pairs left out because a fit failed;
        None in mode 2D.  The result is kept for `summarize_errors()`."""
        if not self.params.useCats:
            raise ValueError("errors() under useCats = 0: a 'wrong class' type has no meaning without categories")
        self.error_eval = error_analysis(self, t_fg, t_bg, area)
        return self.error_eval

    def summarize_errors(self):
        """the table of the last errors(): one line per type with its count and dAP x 100, then the mean Loc pair errors"""
        if getattr(self, "error_eval", None) is None:
            raise Exception("Please run errors() first")
        return "\n".join(error_lines(self._mode, self.params, self.error_eval))


from .drivers import (Omni3DEvaluationHelper, Omni3DEvaluator, _derive_results, inference_on_dataset,  # noqa: F401,E402
                      instances_to_coco_json)
